"""bf16 gather tables on the GPU (spmm_bf16.hip -> SpexGraph.spmm_bf16 / propagate(gather_dtype=torch.bfloat16) -> the drop-in model).

One small square matrix, built here from a seeded generator, takes every path of the kernel: a hub row beyond 1 024 entries
(segments through scratch + the fix-up launch), a 700-entry row (11 segments meeting in LDS), rows of 65 and 64 entries either side
of the task boundary, a block of empty rows, and bin-packed short rows with empty ones among them.  The table is N(0, 1) * 0.05:
almost no entry is representable in bf16, so gathering the fp32 table by mistake cannot pass.

What is checked: the cast against torch's, bit for bit; the product against spex_spmm_f32 on the widened table, BIT FOR BIT, on every
row of at most 1 024 entries and in every form (plain, running sum, add_in, each under both edge-dropout modes); every row, the hub
included, against the fp64 product within the first-order bound of an n-term fp32 fmaf sum in any order; the propagation and its
backward against their launch-by-launch restatements, bit for bit, and against the fp32 propagation within the derived bound (and
NOT equal to it); the drop-in model under SPEX_GATHER_DTYPE=bf16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16 = torch.bfloat16
N, D = 1600, 64
HUB, MID = 1100, 700                 # row 0: beyond kWgRowMax = 1 024; row 1: 11 segments of 64


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ the test graph
def build_csr():
    rng = np.random.default_rng(20240611)
    deg = rng.integers(1, 21, N)
    deg[rng.random(N) < 0.05] = 0                    # empty rows among the short ones
    deg[0], deg[1], deg[2], deg[3] = HUB, MID, 65, 64
    deg[4:10] = 0
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(N, int(k), replace=False)) for k in deg]).astype(np.int32)
    val = (rng.uniform(1e-3, 0.2, len(col)) * rng.choice([-1.0, 1.0], len(col))).astype(np.float32)
    return rowptr.astype(np.int32), col, val


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    from spex_amd.graph import SpexGraph, cast_bf16, csr_transpose
    c = Ctx()
    c.rowptr, c.col, c.val = build_csr()
    c.deg = np.diff(c.rowptr)
    assert c.deg[0] > 1024 and c.deg[1] == 700 and c.deg[2] == 65 and c.deg[3] == 64 and not c.deg[4:10].any()
    assert (c.deg[10:] == 0).any() and c.deg[10:].max() <= 20
    c.graph = SpexGraph(c.rowptr, c.col, c.val)
    t_rowptr, t_col, t_val, eid = csr_transpose(c.rowptr, c.col, c.val, N)
    c.graph_t = SpexGraph(t_rowptr, t_col, t_val, n_cols=N, edge_id=eid)
    gen = torch.Generator().manual_seed(7)
    c.X = (torch.randn(N, D, generator=gen) * 0.05).to(DEV)
    c.X16 = cast_bf16(c.X)
    c.Xw = c.X16.float()
    assert (c.Xw != c.X).float().mean().item() > 0.98                      # almost nothing is representable
    c.E = (torch.randn(N, D, generator=gen) * 0.05).to(DEV)                # epilogue operand (acc_in / add_in)
    c.short = torch.from_numpy(c.deg <= 1024).to(DEV)                      # rows whose sums are bit-identical to the fp32 launch's
    rows = np.repeat(np.arange(N), c.deg)
    A = np.zeros((N, N), np.float64)
    A[rows, c.col] = c.val.astype(np.float64)
    c.A64 = A
    c.keep = (torch.rand(len(c.col), generator=torch.Generator().manual_seed(11)) < 0.3).to(torch.uint8).to(DEV)
    yield c
    c.graph.close()
    c.graph_t.close()


def set_mask(c, mode):
    if mode == 0:
        c.graph.set_edge_mask(0)
    elif mode == 1:
        c.graph.set_edge_mask(1, c.keep, 0.3, 0)
    else:
        c.graph.set_edge_mask(2, None, 0.3, 0x5EED1234)


# ------------------------------------------------------------------------------------------------ 1. cast
def test_cast_equals_torch_bit_for_bit():
    from spex_amd.graph import cast_bf16
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(10007, generator=gen)
    planted = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,      # +-0, +-Inf, NaN
                        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                  # ties above an even / an odd bf16 mantissa
                        0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,                  # either side of a tie; the largest finite -> Inf
                        0x42FE8000, 0x42FF8000], np.uint32).view(np.float32)
    x = torch.cat([torch.from_numpy(planted.copy()), x]).to(DEV)
    nan_at = 4
    for src in (x, x[1:], x[:4 * 1000], x[3:3 + 5]):        # vectorised with a tail, unaligned (scalar kernel), whole vectors, tiny
        want = src.to(BF16)
        got = cast_bf16(src.contiguous())
        finite = ~torch.isnan(src)
        assert torch.equal(bits(got)[finite], bits(want)[finite])
        assert torch.equal(torch.isnan(got.float()), torch.isnan(src))      # NaN stays NaN (not compared by payload)
    got = cast_bf16(x)
    assert torch.isnan(got[nan_at].float())
    want16 = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0, 0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F80, 0xFF80, 0x42FE, 0x4300],
                      np.uint16).view(np.int16)
    sel = [k for k in range(len(want16)) if k != nan_at]
    assert np.array_equal(bits(got)[:len(want16)].cpu().numpy()[sel], want16[sel])


# ------------------------------------------------------------------------------------------------ 2. product, bit identity
FORMS = [("plain", {}), ("acc1", {"acc_div": 1.0}), ("acc4", {"acc_div": 4.0}), ("add4", {"add_div": 4.0}), ("add3", {"add_div": 3.0})]


def run_form(c, form, kw, bf16, with_y16=True, n=N):
    """One launch of `form` -> dict of its outputs.  The running-sum forms also ask for Y (and Y16): every output at once."""
    out = {}
    Y = torch.full((n, D), float("nan"), device=DEV)
    args = {"Y": Y}
    if form.startswith("acc"):
        out["acc_out"] = args["acc_out"] = torch.full((n, D), float("nan"), device=DEV)
        args.update(acc_in=c.E, acc_div=kw["acc_div"])
    elif form.startswith("add"):
        args.update(add_in=c.E, add_div=kw["add_div"])
    if bf16:
        if with_y16:
            out["Y16"] = args["Y16"] = torch.zeros((n, D), dtype=BF16, device=DEV)
        c.graph.spmm_bf16(c.X16, **args)
    else:
        c.graph.spmm(c.Xw, **args)
    out["Y"] = Y
    return out


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["nomask", "keepmask", "sampled"])
@pytest.mark.parametrize("form,kw", FORMS, ids=[f[0] for f in FORMS])
def test_product_is_the_fp32_launch_on_the_widened_table_bit_for_bit(ctx, form, kw, mode):
    c = ctx
    set_mask(c, mode)
    try:
        ref = run_form(c, form, kw, bf16=False)
        got = run_form(c, form, kw, bf16=True)
        again = run_form(c, form, kw, bf16=True)
    finally:
        c.graph.set_edge_mask(0)
    for k in ref:
        assert not torch.isnan(got[k]).any(), f"{form}: rows of {k} were not written"
        assert torch.equal(bits(got[k])[c.short], bits(ref[k])[c.short]), f"{form} mode {mode}: {k} differs from spex_spmm_f32 on Xw"
    assert same_bits(got["Y16"], got["Y"].to(BF16)), f"{form}: Y16 is not bf16(Y)"
    for k in got:
        assert same_bits(got[k], again[k]), f"{form}: two runs differ in {k}"
    # rows without stored entries: 0, or the epilogue's value
    empty = torch.from_numpy(c.deg == 0).to(DEV)
    if form == "plain":
        assert (got["Y"][empty] == 0).all() and (bits(got["Y16"])[empty] == 0).all()
    elif form.startswith("acc"):
        assert (got["Y"][empty] == 0).all()
        assert torch.equal(got["acc_out"][empty], c.E[empty] / kw["acc_div"])       # (/1 and /4: exact)
    elif form == "add4":
        assert torch.equal(got["Y"][empty], c.E[empty] / 4.0)


def test_adjacent_row_tasks_of_a_table_beyond_the_caches_bit_for_bit():
    """The ROWIDS = false instantiations (a task's rows adjacent from task.z: tables whose fp32 source exceeds 16 MiB, n_cols > 65 536),
    which the square graph above — bin-packed, 1 600 columns — never launches: 400 x 70 000, degrees 0..63 with rows of 0, 1, 64, 65,
    700, 1 024 and 1 025 entries planted, every form under every mask mode."""
    from spex_amd.graph import SpexGraph, cast_bf16
    n_rows, n_cols = 400, 70000
    rng = np.random.default_rng(70000)
    deg = rng.integers(0, 64, n_rows)
    deg[:7] = [0, 1, 64, 65, 700, 1024, 1025]
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n_cols, int(k), replace=False)) for k in deg]).astype(np.int32)
    val = (rng.uniform(1e-3, 0.2, len(col)) * rng.choice([-1.0, 1.0], len(col))).astype(np.float32)
    c = Ctx()
    c.graph = SpexGraph(rowptr.astype(np.int32), col, val, n_cols=n_cols)
    try:
        gen = torch.Generator().manual_seed(17)
        c.X16 = cast_bf16((torch.randn(n_cols, D, generator=gen) * 0.05).to(DEV))
        c.Xw = c.X16.float()
        c.E = (torch.randn(n_rows, D, generator=gen) * 0.05).to(DEV)
        c.keep = (torch.rand(len(col), generator=torch.Generator().manual_seed(11)) < 0.3).to(torch.uint8).to(DEV)
        short = torch.from_numpy(deg <= 1024).to(DEV)
        assert int((~short).sum()) == 1
        for mode in (0, 1, 2):
            set_mask(c, mode)
            for form, kw in FORMS:
                ref = run_form(c, form, kw, bf16=False, n=n_rows)
                got = run_form(c, form, kw, bf16=True, n=n_rows)
                again = run_form(c, form, kw, bf16=True, n=n_rows)
                for k in ref:
                    assert not torch.isnan(got[k]).any(), f"{form} mode {mode}: rows of {k} were not written"
                    assert torch.equal(bits(got[k])[short], bits(ref[k])[short]), f"{form} mode {mode}: {k} differs from spex_spmm_f32 on Xw"
                assert same_bits(got["Y16"], got["Y"].to(BF16)), f"{form} mode {mode}: Y16 is not bf16(Y)"
                for k in got:
                    assert same_bits(got[k], again[k]), f"{form} mode {mode}: two runs differ in {k}"
    finally:
        c.graph.close()


def test_single_outputs_match_the_all_outputs_launch(ctx):
    """Y16 alone (the propagation's middle layers), acc_out alone (its last), and the allocate-Y default."""
    c = ctx
    full = run_form(c, "acc4", {"acc_div": 4.0}, bf16=True)
    y16 = torch.zeros((N, D), dtype=BF16, device=DEV)
    assert c.graph.spmm_bf16(c.X16, Y16=y16) is y16 and same_bits(y16, full["Y16"])
    acc = torch.empty((N, D), device=DEV)
    assert c.graph.spmm_bf16(c.X16, acc_in=c.E, acc_out=acc, acc_div=4.0) is acc and same_bits(acc, full["acc_out"])
    assert same_bits(c.graph.spmm_bf16(c.X16), full["Y"])
    with pytest.raises(ValueError):
        c.graph.spmm_bf16(c.Xw)                                                      # an fp32 table is refused, not converted
    from spex_amd._lib import SpexError
    with pytest.raises(SpexError, match="d == 64"):
        c.graph.spmm_bf16(torch.zeros((N, 32), dtype=BF16, device=DEV))


# ------------------------------------------------------------------------------------------------ 3. product, independent truth
def test_product_within_the_fmaf_sum_bound_of_the_fp64_product_on_every_row(ctx):
    c = ctx
    Xw64 = c.Xw.cpu().numpy().astype(np.float64)
    y64 = c.A64 @ Xw64
    mag = np.abs(c.A64) @ np.abs(Xw64)
    bound = (c.deg[:, None] + 2) * 2.0 ** -24 * mag
    y16 = torch.zeros((N, D), dtype=BF16, device=DEV)
    Y = c.graph.spmm_bf16(c.X16, Y=torch.empty((N, D), device=DEV), Y16=y16).cpu().numpy().astype(np.float64)
    err = np.abs(Y - y64)
    worst = int(np.argmax((err / np.maximum(bound, 1e-300)).max(axis=1)))
    print(f"max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f} at row {worst} ({c.deg[worst]} entries); hub row: "
          f"{(err[0] / bound[0]).max():.3f}")
    assert (err <= bound).all()
    assert same_bits(y16, torch.from_numpy(Y.astype(np.float32)).to(DEV).to(BF16))      # the hub row's Y16 too


# ------------------------------------------------------------------------------------------------ 4. propagate
def restate_fwd(graph, E0, L):
    """spex_propagate_bf16_f32 launch by launch: cast, then L launches with Y16 and acc_out."""
    from spex_amd.graph import cast_bf16
    if L == 0:
        return E0.clone()
    cur, out = cast_bf16(E0), torch.empty_like(E0)
    for l in range(L):
        last = l == L - 1
        nxt = None if last else torch.empty_like(cur)
        graph.spmm_bf16(cur, Y16=nxt, acc_in=E0 if l == 0 else out, acc_out=out, acc_div=float(L + 1) if last else 1.0)
        cur = nxt
    return out


def restate_bwd(graph_t, g_out, L):
    """spex_propagate_bwd_bf16_f32 launch by launch: gs = g / (L+1) (correctly rounded fp32 division, done on the host), its
    rounding as the first gather source, then L launches in the add_in form on the transposed handle."""
    from spex_amd.graph import cast_bf16
    if L == 0:
        return g_out.clone()
    gs = torch.from_numpy(g_out.cpu().numpy() / np.float32(L + 1)).to(g_out.device)
    cur, out = cast_bf16(gs), torch.empty_like(g_out)
    for l in range(L - 1, -1, -1):
        last = l == 0
        nxt = None if last else torch.empty_like(cur)
        graph_t.spmm_bf16(cur, Y=out if last else None, Y16=nxt, add_in=gs, add_div=1.0)
        cur = nxt
    return out


@pytest.mark.parametrize("L", [1, 2, 3])
def test_propagate_equals_its_restatement_and_stays_within_the_bound_of_fp32(ctx, L):
    c = ctx
    E0 = c.X
    got = c.graph.propagate(E0, L, gather_dtype=BF16)
    assert same_bits(got, restate_fwd(c.graph, E0, L))
    assert same_bits(got, c.graph.propagate(E0, L, gather_dtype=BF16))
    ref = c.graph.propagate(E0, L)
    assert same_bits(ref, c.graph.propagate(E0, L, gather_dtype=torch.float32))      # fp32 by name is today's path
    # |mean16 - mean32| <= sum_l l 2^-8 (|A|^l |E0|) / (L+1): unit roundoff 2^-9 per rounded gather source, compounding once per
    # layer, a factor 2 over first order for the fp32 accumulation and the second-order terms
    absA, P = np.abs(c.A64), np.abs(E0.cpu().numpy().astype(np.float64))
    bound = np.zeros((N, D))
    for l in range(1, L + 1):
        P = absA @ P
        bound += l * 2.0 ** -8 * P
    bound /= L + 1
    dev = np.abs(got.cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64))
    print(f"L = {L}: max |bf16 - fp32| = {dev.max():.3e}, max dev / bound = {(dev / np.maximum(bound, 1e-300)).max():.3f}")
    assert (dev <= bound).all()
    assert dev.max() > 0 and (dev > 0).mean() > 0.5             # the bf16 table is what was gathered
    with pytest.raises(ValueError, match="gather_dtype"):
        c.graph.propagate(E0, L, gather_dtype=torch.float16)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_propagate_bwd_equals_its_restatement(ctx, L):
    c = ctx
    g = c.E
    got = c.graph_t.propagate_bwd(g, L, gather_dtype=BF16)
    assert same_bits(got, restate_bwd(c.graph_t, g, L))
    ref = c.graph_t.propagate_bwd(g, L)
    assert not torch.equal(got, ref)
    # straight-through: the fp32 backward up to the rounding of its gather sources (the forward bound, on A^T)
    absA, P = np.abs(c.A64.T), np.abs(g.cpu().numpy().astype(np.float64))
    bound = np.zeros((N, D))
    for l in range(1, L + 1):
        P = absA @ P
        bound += l * 2.0 ** -8 * P
    bound /= L + 1
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref.cpu().numpy().astype(np.float64)) <= bound).all()
    with pytest.raises(ValueError, match="gather_dtype"):
        c.graph_t.propagate_bwd(g, L, gather_dtype="bf16")


def test_propagate_zero_layers_is_the_identity(ctx):
    assert same_bits(ctx.graph.propagate(ctx.X, 0, gather_dtype=BF16), ctx.X)
    assert same_bits(ctx.graph_t.propagate_bwd(ctx.E, 0, gather_dtype=BF16), ctx.E)


# ------------------------------------------------------------------------------------------------ 5. autograd and drop-in
@pytest.fixture(scope="module")
def data_root(tmp_path_factory, golden):
    from spex_amd.datasets import materialise_rating_files
    g = golden("lightgcn_tiny")
    return materialise_rating_files(str(tmp_path_factory.mktemp("data")), "tiny", g["train_pairs"], g["test_users"], g["test_pos"],
                                    g["test_neg"])


def build(data_root, extra=()):
    import lg_parser
    import utility1.dataloader as dataloader
    import utility1.model as model
    import utility1.utils as utils
    args = lg_parser.parse_args_r(["--dataset", "tiny", "--data_path", data_root, *extra])
    utils.set_seed(args.seed)
    dataset = dataloader.Loader(args)
    return model.LightGCN(args, dataset).to(DEV)


def flat(net):
    return torch.cat([net.embedding_user.weight, net.embedding_item.weight]).detach()


def test_dropin_model_gathers_bf16_when_asked(data_root, golden, monkeypatch):
    from spex_amd import ops
    g = golden("lightgcn_tiny")
    bu, bi, bl = (torch.from_numpy(g[k][0]) for k in ("batch_users", "batch_items", "batch_labels"))
    monkeypatch.setenv("SPEX_GATHER_DTYPE", "bf16")
    net16 = build(data_root)
    assert net16.gather_dtype == BF16
    with pytest.raises(ValueError, match="A_split"):
        build(data_root, ["--A_split", "1", "--a_fold", "7"])
    monkeypatch.setenv("SPEX_GATHER_DTYPE", "fp16")
    with pytest.raises(ValueError, match="SPEX_GATHER_DTYPE"):
        build(data_root)
    monkeypatch.delenv("SPEX_GATHER_DTYPE")
    net32 = build(data_root)
    assert net32.gather_dtype == torch.float32
    E0, L = flat(net16), net16.n_layers
    assert same_bits(E0, flat(net32))

    # computer(), flag = 1 scoring and the eval cache all read the bf16 propagation
    want = net16.Graph.propagate(E0, L, gather_dtype=BF16).clone()
    net16.eval()
    with torch.no_grad():
        out16 = torch.cat(net16.computer())
        assert same_bits(out16, want) and same_bits(out16, restate_fwd(net16.Graph, E0, L))
        assert net16._light_out().data_ptr() == net16._light_out().data_ptr()            # cached
        n_u = net16.num_users + 1
        gamma = net16(bu, bi, None, flag=1)
        gamma_want, _ = ops.score_bce(want[:n_u], want[n_u:], bu, bi)
        assert same_bits(gamma, gamma_want)
    # a model built without the variable is today's: the reference's golden table, bit for bit
    net32.eval()
    with torch.no_grad():
        out32 = torch.cat(net32.computer())
    assert np.array_equal(out32.cpu().numpy(), g["light_out"]) and same_bits(out32, net32.Graph.propagate(E0, L))
    assert not torch.equal(out16, out32)

    # training node (forward(flag=0): LightGCNBCELoss): the bf16 model's table gradients are what the fp32 model computes once its
    # propagation is replaced by the bf16 restatement — bit for bit in the deterministic mode (no float atomics)
    monkeypatch.setattr(net32.Graph, "propagate", lambda E, n_layers, **kw: restate_fwd(net32.Graph, E, n_layers), raising=False)
    monkeypatch.setattr(net32.Graph, "propagate_bwd", lambda gr, n_layers, **kw: restate_bwd(net32.Graph, gr, n_layers), raising=False)
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        res = []
        for net in (net16, net32):
            net.train()
            net.zero_grad()
            loss = net(bu, bi, bl, flag=0)
            loss.backward()
            res.append((loss.detach().clone(), torch.cat([net.embedding_user.weight.grad, net.embedding_item.weight.grad]).clone()))
        # (the loss is a sum of B per-sample terms by float atomics, whose order varies from launch to launch: the terms are the same
        #  bits, so two sums differ by at most the first-order bound of a B-term fp32 sum in any order, B 2^-24 sum|l_b| — on the mean,
        #  B 2^-24 times the mean itself; the GRADIENT rows are added in slot order in this mode)
        l0, l1 = res[0][0].item(), res[1][0].item()
        assert abs(l0 - l1) <= bu.numel() * 2.0 ** -24 * abs(l1)
        assert same_bits(res[0][1], res[1][1]) and res[0][1].abs().max().item() > 0
        # computer() under autograd (PropagateMean: what bpr_loss and the flag = 0 fallback read): table and gradient, bit for bit
        w = torch.randn(want.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        net16.zero_grad()
        out = torch.cat(net16.computer())
        assert out.requires_grad and same_bits(out.detach(), want)
        (out * w).sum().backward()
        g16 = torch.cat([net16.embedding_user.weight.grad, net16.embedding_item.weight.grad])
        assert same_bits(g16, restate_bwd(net16.Graph, w, L))
        # bpr_loss reads the same node (its scoring kernel adds with float atomics, whose order varies from launch to launch: the
        # losses of the two models are compared to 1e-6, as the drop-in tests compare such losses)
        pos, neg = torch.from_numpy(g["batch_items"][0]), torch.from_numpy(np.roll(g["batch_items"][0], 1))
        l16, l32 = net16.bpr_loss(bu, pos, neg)[0].item(), net32.bpr_loss(bu, pos, neg)[0].item()
        assert np.isfinite(l16) and abs(l16 - l32) <= 1e-6
    finally:
        ops.set_deterministic(was)
