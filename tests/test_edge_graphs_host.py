"""Graphs (f) and (g) and their per-edge inputs, in NumPy alone: the inputs of tests/test_gpu_edge_regimes.py, and the proof that they
cross every grid cap and softmax tile edge of DESIGN.md 4.26 — so that a later edit of a generator cannot silently move those tests
back under a cap.

Graph (f): 140 000 x 135 000, ~5.1 M entries, columns sorted and distinct per row (one column per equal-width bin of [0, n_cols)).
Rows 0 .. 11 have 0, 1, 16, 17, 64, 65, 1 025, 1 024, 1 000, 883, 1 024 and 5 000 entries: the 1 025-entry hub is entries 163 .. 1 187 of
tile 0 with ordinary rows after it in that tile; row 10 (1 024 entries) starts at entry 4 095, the last of tile 1; the 5 000-entry hub starts
in tile 2, covers all of tile 3 and ends in tile 4.  Then 6 000 rows of 0, 1, 1, 0, 2 entries in turn (a 2 048-entry tile inside the run has
2 560 row starts), background rows of 30 .. 46 entries, and the last three rows: empty, 5 entries, empty.  Column 777 is stored in 1 200
background rows, so the transposed pattern has a hub too.

Graph (g): 9 000 x 7 000, ~32 000 entries (the 512 tile).  Rows 0 .. 9 have 0, 1, 16, 17, 64, 65, 348, 1 024, 1 025 and 700 entries: row 7
(1 024 entries) starts at entry 511, the last of tile 0.  Then 4 000 rows of 0, 0, 1, 0, 1 entries in turn (1 280 row starts in one 512
tile), background rows of 0 .. 11 entries.  Column 3 is stored in 1 100 background rows and column 5 in 300, so the transposed pattern
has a hub and a mid row.

Per-edge inputs: 3 N(0, 1), with 90 + N(0, 1) planted into a short row (<= 16 entries), a mid row and a hub row, and -90 + N(0, 1) into
another row of each class: expf(90) overflows fp32, so a kernel that drops the row maximum yields inf or NaN.
"""
import numpy as np

# the bounds of DESIGN.md 4.26, read from the kernels
SOFTMAX_TILE = 2048                        # spex_common.h:168 kSoftmaxTile
SMALL_TILE = 512                           # graph.hip:633: the tile while nnz / 2 048 < 2 048
TILE_SWITCH_NNZ = 2048 * 2048              # graph.hip:633: 4 194 304 entries
WG_ROW_MAX = 1024                          # spex_common.h:162 kWgRowMax; edge.hip:161: rows beyond it go to the hub kernel
TILE_ROW_CAP = 1024                        # edge.hip:123 kTileRowCap; edge.hip:154-160: later rows read rowptr from memory
STREAM_THREADS = 256 * 32 * 256            # edge.hip:247-253 stream_grid: 8 192 workgroups of 256 threads
ROW_OF_ROWS = STREAM_THREADS // 16         # edge.hip:60-67 row_of_kernel: 16 lanes per row, 131 072 rows per trip
CHUNK = 16                                 # spex_common.h:164 kChunk: 16 n_chunks >= nnz entries in the chunk copy
ROW_IDS_MAX_COLS = 65536                   # graph.hip:245: row ids while n_cols x 256 B <= 16 MiB; beyond: adjacent rows
FUSE_ROWS = 256 * 16                       # fuse.hip:186-191 fuse_grid: 256 workgroups x 16 waves, a row per wave and trip

F_ROWS, F_COLS = 140000, 135000
F_PREFIX = [0, 1, 16, 17, 64, 65, 1025, 1024, 1000, 883, 1024, 5000]
F_RUN, F_CYCLE = 6000, [0, 1, 1, 0, 2]
F_BG = (30, 47)                            # background degrees, integers(lo, hi)
F_HUB_COL, F_HUB_COL_ROWS = 777, 1200
G_ROWS, G_COLS = 9000, 7000
G_PREFIX = [0, 1, 16, 17, 64, 65, 348, 1024, 1025, 700]
G_RUN, G_CYCLE = 4000, [0, 0, 1, 0, 1]
G_BG = (0, 12)
G_HUB_COL, G_HUB_COL_ROWS, G_MID_COL, G_MID_COL_ROWS = 3, 1100, 5, 300
# rows the inputs plant +90 / -90 into: (short, mid, hub) each; (g) has one hub: it takes both signs, half each
F_PLANT = {"hot": (2, 7, 6), "cold": (F_ROWS - 2, 8, 11)}
G_PLANT = {"hot": (2, 7, 8), "cold": (G_ROWS - 1, 9, 8)}
FUSE_N = 2 * FUSE_ROWS + 17                # attn_fuse rows of Part C: two full trips and a ragged one
MODEL_U, MODEL_I = 4200, 4300              # Part D: both fuse launches stride
_cache = {}


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def stratified_csr(rng, deg, n_cols):
    """(rowptr, col): row r holds deg[r] sorted distinct columns, entry j in bin [j w, (j + 1) w), w = n_cols // deg[r]."""
    deg = np.asarray(deg, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    rows = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    j = np.arange(rowptr[-1], dtype=np.int64) - rowptr[rows]
    w = n_cols // deg[rows]
    col = j * w + rng.integers(0, 1 << 30, len(j)) % w
    assert rowptr[-1] < 2 ** 31
    return rowptr.astype(np.int32), col.astype(np.int32)


def graph_f():
    """(rowptr, col, val) of graph (f)."""
    if "f" not in _cache:
        rng = np.random.default_rng(26)
        n_bg = F_ROWS - len(F_PREFIX) - F_RUN - 3
        deg = np.concatenate([F_PREFIX, np.resize(F_CYCLE, F_RUN), rng.integers(*F_BG, n_bg), [0, 5, 0]])
        rowptr, col = stratified_csr(rng, deg, F_COLS)
        first_bg = len(F_PREFIX) + F_RUN
        hub_rows = first_bg + rng.choice(n_bg, F_HUB_COL_ROWS, replace=False)
        col[rowptr[hub_rows]] = F_HUB_COL              # a row's first entry lies in [0, w), w >= 135 000 // 46 > 777: still sorted
        val = rng.standard_normal(len(col), dtype=np.float32)
        _cache["f"] = (rowptr, col, val)
    return _cache["f"]


def graph_g():
    """(rowptr, col, val) of graph (g)."""
    if "g" not in _cache:
        rng = np.random.default_rng(27)
        n_bg = G_ROWS - len(G_PREFIX) - G_RUN
        deg = np.concatenate([G_PREFIX, np.resize(G_CYCLE, G_RUN), rng.integers(*G_BG, n_bg)])
        deg[-1] = 7                                    # the last row is not empty (and is the short row that takes -90)
        rowptr, col = stratified_csr(rng, deg, G_COLS)
        first_bg = len(G_PREFIX) + G_RUN
        picked = first_bg + rng.permutation(np.flatnonzero(deg[first_bg:] > 0))[:G_HUB_COL_ROWS + G_MID_COL_ROWS]
        col[rowptr[picked[:G_HUB_COL_ROWS]]] = G_HUB_COL           # first entries lie in [0, w), w >= 7 000 // 11 > 5: still sorted
        col[rowptr[picked[G_HUB_COL_ROWS:]]] = G_MID_COL
        _cache["g"] = (rowptr, col, rng.standard_normal(len(col), dtype=np.float32))
    return _cache["g"]


def transpose(csr, n_cols):
    """spex_amd.graph.csr_transpose restated: (t_rowptr, t_col, t_val, perm), perm[k] = the entry of A that A^T's entry k is."""
    rowptr, col, val = csr
    order = np.argsort(col, kind="stable")             # entries are row-major: a stable sort by column keeps the rows ascending
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int32)
    return t_rowptr, rows_of(rowptr)[order].astype(np.int32), val[order], order.astype(np.int32)


def transposed(which):
    if ("t", which) not in _cache:
        _cache["t", which] = transpose(graph_f(), F_COLS) if which == "f" else transpose(graph_g(), G_COLS)
    return _cache["t", which]


def tile_rows(rowptr, tile):
    """graph.hip:634-643 restated: tile_row[t] = the first row that starts at or after entry t x tile."""
    nnz, n = int(rowptr[-1]), len(rowptr) - 1
    n_tiles = (nnz + tile - 1) // tile
    return np.searchsorted(rowptr[:n], np.arange(n_tiles + 1, dtype=np.int64) * tile, side="left")


def tile_of(nnz):
    return SMALL_TILE if nnz // SOFTMAX_TILE < 2048 else SOFTMAX_TILE


def plant_rows(rowptr):
    """Rows to plant into on a pattern without named rows (a transposed one): the first short (2 .. 16 entries), mid (17 .. 1 024) and
    hub row for +90, the last of each class for -90 (a class with one row gives it both signs, half each)."""
    deg = np.diff(rowptr)
    classes = [np.flatnonzero((deg >= 2) & (deg <= 16)), np.flatnonzero((deg > 16) & (deg <= WG_ROW_MAX)), np.flatnonzero(deg > WG_ROW_MAX)]
    assert all(len(c) for c in classes), [len(c) for c in classes]
    return {"hot": tuple(int(c[0]) for c in classes), "cold": tuple(int(c[-1]) for c in classes)}


def planted_inputs(rowptr, plant, seed):
    """Per-entry softmax input in the pattern's entry order: 3 N(0, 1); 90 + N(0, 1) on the `hot` rows, -90 + N(0, 1) on the `cold`
    ones (a row named in both: its first half hot, its second half cold)."""
    rng = np.random.default_rng(seed)
    v = 3.0 * rng.standard_normal(int(rowptr[-1]))
    for r in plant["hot"]:
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        e = b + (e - b) // 2 if r in plant["cold"] else e
        v[b:e] = 90.0 + rng.standard_normal(e - b)
    for r in plant["cold"]:
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        b = b + (e - b) // 2 if r in plant["hot"] else b
        v[b:e] = -90.0 + rng.standard_normal(e - b)
    return v.astype(np.float32)


def softmax_fp64(rowptr, v):
    """Row softmax over the stored entries in fp64 (np.reduceat over the non-empty rows)."""
    v = np.asarray(v, np.float64)
    deg = np.diff(rowptr)
    starts = rowptr[:-1][deg > 0].astype(np.int64)
    lens = deg[deg > 0]
    e = np.exp(v - np.repeat(np.maximum.reduceat(v, starts), lens))
    return e / np.repeat(np.add.reduceat(e, starts), lens)


def softmax_bwd_fp64(rowptr, y, gy):
    y, gy = np.asarray(y, np.float64), np.asarray(gy, np.float64)
    deg = np.diff(rowptr)
    starts = rowptr[:-1][deg > 0].astype(np.int64)
    return y * (gy - np.repeat(np.add.reduceat(y * gy, starts), deg[deg > 0]))


def block_rows(which):
    """The rows of the small handle the tile-independence tests hold the big one against: the prefix and the run, a background block,
    the last 300 rows."""
    n, first_bg = (F_ROWS, len(F_PREFIX) + F_RUN) if which == "f" else (G_ROWS, len(G_PREFIX) + G_RUN)
    return np.concatenate([np.arange(first_bg), np.arange(first_bg + 700, first_bg + 1200), np.arange(n - 300, n)])


def take_rows(csr, rows):
    """(rowptr, col, val, entries): the listed rows of a CSR matrix as a matrix of their own; entries = their entries in the source."""
    rowptr, col, val = csr
    lens = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    new_ptr = np.concatenate([[0], np.cumsum(lens)])
    e = np.repeat(rowptr[rows].astype(np.int64) - new_ptr[:-1], lens) + np.arange(new_ptr[-1])
    return new_ptr.astype(np.int32), col[e], val[e], e


# ------------------------------------------------------------------------------------------ the properties
def check_pattern(csr, n_rows, n_cols):
    rowptr, col, val = csr
    assert len(rowptr) == n_rows + 1 and rowptr[0] == 0 and rowptr[-1] == len(col) == len(val)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert col.min() >= 0 and col.max() < n_cols
    rows = rows_of(rowptr)
    key = rows * n_cols + col
    assert (np.diff(key) > 0).all()                     # row-major, columns sorted and distinct per row
    return np.diff(rowptr)


def tile_facts(rowptr, tile):
    """What the softmax tile kernel meets on this pattern, from rowptr alone."""
    deg = np.diff(rowptr)
    tr = tile_rows(rowptr, tile)
    starts = np.diff(tr)
    assert tr[0] == 0 and (np.diff(tr) >= 0).all()
    facts = {"max_starts": int(starts.max()), "no_start": bool((starts == 0).any())}
    # a tile with more than kTileRowCap starts whose rows past the 1 024th include non-empty ones
    facts["late_rows_with_entries"] = any(deg[tr[t] + TILE_ROW_CAP:tr[t + 1]].any() for t in np.flatnonzero(starts > TILE_ROW_CAP))
    # a non-hub row of exactly kWgRowMax entries that starts on a tile's last entry: staged up to cap - 1
    full = np.flatnonzero(deg == WG_ROW_MAX)
    facts["full_row_at_last_offset"] = bool((rowptr[full] % tile == tile - 1).any())
    # a hub that starts and ends inside one tile, with a row start after it in that tile
    hubs = np.flatnonzero(deg > WG_ROW_MAX)
    inside = hubs[rowptr[hubs] // tile == (rowptr[hubs + 1] - 1) // tile]
    facts["hub_then_row_start"] = any(rowptr[h + 1] // tile == rowptr[h] // tile and h + 1 < len(deg) for h in inside)
    # a hub whose tile's e_hi is clipped to cap = (t + 1) tile + kWgRowMax: the hub is the last row that starts in its tile
    facts["clipped_hub"] = any(rowptr[h + 1] > (rowptr[h] // tile + 1) * tile + WG_ROW_MAX and tr[rowptr[h] // tile + 1] == h + 1 for h in hubs)
    return facts


def test_graph_f_crosses_every_cap():
    rowptr, col, val = graph_f()
    deg = check_pattern(graph_f(), F_ROWS, F_COLS)
    nnz = int(rowptr[-1])
    assert list(deg[:len(F_PREFIX)]) == F_PREFIX and list(deg[-3:]) == [0, 5, 0]
    assert list(rowptr[:13]) == [0, 0, 1, 17, 34, 98, 163, 1188, 2212, 3212, 4095, 5119, 10119]
    run = deg[len(F_PREFIX):len(F_PREFIX) + F_RUN]
    assert list(run[:10]) == F_CYCLE * 2 and run.sum() == F_RUN // 5 * 4
    bg = deg[len(F_PREFIX) + F_RUN:-3]
    assert bg.min() >= 30 and bg.max() <= 46
    # the production tile, with a margin of a sixth
    assert nnz // SOFTMAX_TILE >= 2048 and nnz >= TILE_SWITCH_NNZ * 7 // 6 and tile_of(nnz) == SOFTMAX_TILE
    # stream_grid: every loop of set_values_kernel that a rectangular handle runs, and row_of_kernel, take a second trip (the chunk copy
    # holds 16 n_chunks >= nnz entries)
    assert nnz > 2 * STREAM_THREADS and CHUNK * F_ROWS > STREAM_THREADS
    assert F_ROWS > ROW_OF_ROWS and F_COLS > ROW_OF_ROWS
    # the adjacent-row layout on the handle and on its transposed copy
    assert F_COLS > ROW_IDS_MAX_COLS and F_ROWS > ROW_IDS_MAX_COLS
    facts = tile_facts(rowptr, SOFTMAX_TILE)
    assert facts == {"max_starts": 2560, "no_start": True, "late_rows_with_entries": True, "full_row_at_last_offset": True,
                     "hub_then_row_start": True, "clipped_hub": True}, facts
    tr = tile_rows(rowptr, SOFTMAX_TILE)
    assert tr[3] == tr[4] == 12                         # tile 3 lies inside the 5 000-entry row
    assert rowptr[6] // 2048 == (rowptr[7] - 1) // 2048 == 0 and rowptr[10] == 2 * 2048 - 1 and rowptr[11] // 2048 == 2 and (rowptr[12] - 1) // 2048 == 4


def test_graph_f_transposed_has_a_hub_and_the_same_regime():
    t_rowptr, t_col, t_val, perm = transposed("f")
    deg = check_pattern((t_rowptr, t_col, t_val), F_COLS, F_ROWS)
    assert deg[F_HUB_COL] >= 1100 and deg.max() > WG_ROW_MAX
    assert tile_of(int(t_rowptr[-1])) == SOFTMAX_TILE
    assert np.array_equal(np.sort(perm), np.arange(len(perm)))
    rowptr, col, val = graph_f()
    assert np.array_equal(col[perm], rows_of(t_rowptr)) and np.array_equal(rows_of(rowptr)[perm], t_col) and np.array_equal(val[perm], t_val)
    plant = plant_rows(t_rowptr)
    assert deg[plant["hot"][2]] > WG_ROW_MAX


def test_transpose_is_the_librarys():
    from spex_amd.graph import csr_transpose
    for csr, n_cols, which in ((graph_g(), G_COLS, "g"), (take_rows(graph_f(), block_rows("f"))[:3], F_COLS, None)):
        want = csr_transpose(*csr, n_cols)
        got = transposed(which) if which else transpose(csr, n_cols)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(want, got))


def test_graph_g_meets_the_same_edges_at_the_512_tile():
    rowptr, col, val = graph_g()
    deg = check_pattern(graph_g(), G_ROWS, G_COLS)
    nnz = int(rowptr[-1])
    assert list(deg[:len(G_PREFIX)]) == G_PREFIX
    assert list(rowptr[:11]) == [0, 0, 1, 17, 34, 98, 163, 511, 1535, 2560, 3260]
    assert list(deg[len(G_PREFIX):len(G_PREFIX) + 10]) == G_CYCLE * 2
    assert nnz // SOFTMAX_TILE < 2048 and tile_of(nnz) == SMALL_TILE and 28000 <= nnz <= 36000
    assert G_COLS <= ROW_IDS_MAX_COLS                   # the layout with row ids
    facts = tile_facts(rowptr, SMALL_TILE)
    # (a hub cannot begin and end inside a 512 tile)
    assert facts == {"max_starts": 1280, "no_start": True, "late_rows_with_entries": True, "full_row_at_last_offset": True,
                     "hub_then_row_start": False, "clipped_hub": False}, facts
    assert rowptr[7] == SMALL_TILE - 1 and deg[7] == WG_ROW_MAX


def test_row_blocks_keep_every_row_form_and_run_the_small_tile():
    for which, csr, plant in (("f", graph_f(), F_PLANT), ("g", graph_g(), G_PLANT)):
        rows = block_rows(which)
        rowptr, col, val, e = take_rows(csr, rows)
        assert len(np.unique(rows)) == len(rows) and tile_of(len(col)) == SMALL_TILE
        assert np.array_equal(np.diff(rowptr), np.diff(csr[0])[rows]) and np.array_equal(col, csr[1][e])
        assert all(r in rows for r in plant["hot"] + plant["cold"])
        assert which == "f" or tile_facts(rowptr, SMALL_TILE)["max_starts"] > TILE_ROW_CAP


def test_planted_inputs_overflow_without_the_row_maximum_and_their_fp64_softmax_is_finite():
    cases = [(graph_f()[0], F_PLANT), (graph_g()[0], G_PLANT)]
    for which in ("f", "g"):
        t_rowptr = transposed(which)[0]
        cases.append((t_rowptr, plant_rows(t_rowptr)))
    for k, (rowptr, plant) in enumerate(cases):
        deg = np.diff(rowptr)
        for rows in (plant["hot"], plant["cold"]):
            assert 2 <= deg[rows[0]] <= 16 and 16 < deg[rows[1]] <= WG_ROW_MAX and deg[rows[2]] > WG_ROW_MAX, (k, deg[list(rows)])
        v = planted_inputs(rowptr, plant, 40 + k)
        assert v.dtype == np.float32 and len(v) == rowptr[-1]
        with np.errstate(over="ignore"):
            for r in plant["hot"]:                      # expf(90) overflows fp32: without the row maximum the row's sum is inf
                assert np.isinf(np.exp(v[rowptr[r]:rowptr[r + 1]])).any()
        assert all((v[rowptr[r]:rowptr[r + 1]] > 80).any() for r in plant["hot"])
        assert all((v[rowptr[r]:rowptr[r + 1]] < -80).any() for r in plant["cold"])
        y = softmax_fp64(rowptr, v)
        assert np.isfinite(y).all() and y.min() >= 0
        sums = np.add.reduceat(y, rowptr[:-1][deg > 0].astype(np.int64))
        assert np.abs(sums - 1.0).max() <= 1e-12
        assert (y[rowptr[:-1][deg == 1]] == 1.0).all()
        gx = softmax_bwd_fp64(rowptr, y, np.random.default_rng(k).standard_normal(len(y)))
        assert np.isfinite(gx).all() and not gx[rowptr[:-1][deg == 1]].any()


def test_fused_rows_make_two_full_trips_and_a_ragged_one():
    assert FUSE_N == 2 * FUSE_ROWS + 17 and MODEL_U > FUSE_ROWS and MODEL_I > FUSE_ROWS
