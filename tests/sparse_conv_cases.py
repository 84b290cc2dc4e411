"""Seeded cases and float64 references of the op-level tests of csrc/sparse_conv.hip, shared by tests/test_sparse_conv_cpu.py
-- which pins the references against the dense oracle (oracle/cpu_backend.py::sparse_conv3d_dense) with no kernel involved
and checks that the device bound is satisfiable -- and tests/test_sparse_conv_edges_gpu.py.

numpy and Python only.  The rulebook reference restates the definition with a dict (b, z, y, x) -> row and never
densifies, so it works at the shipped grid (41, 1600, 1408) as well.  Every case names the code path it is there for.

The bound of every value comparison is per ELEMENT: |got - ref| <= gamma(n + m) * S + 1e-30 with S = sum |a| |b| over the
products of that element, n their number, m the extra additions of the kernel (2 for forward / data gradient, partials + 2
for the weight gradient), gamma(x) = x u / (1 - x u), u = 2^-24: the forward-error bound of an fp32 sum in ANY order
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); zero-padded terms add exactly."""
import itertools

import numpy as np

U = 2.0 ** -24


def gamma(x):
    x = np.asarray(x, np.float64)
    return x * U / (1.0 - x * U)


def bound(n, m, S):
    return gamma(np.asarray(n, np.float64) + m) * S + 1e-30


def triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


# ------------------------------------------------------------------------------------------------ rulebook reference
def site_table(coords, shape):
    """(b, z, y, x) -> row over the in-grid rows with b >= 0; a duplicated coordinate keeps its smallest row (csrc/voxel_hash.hpp)."""
    table = {}
    for r, (b, z, y, x) in enumerate(np.asarray(coords).reshape(-1, 4).tolist()):
        if b >= 0 and 0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2]:
            table.setdefault((b, z, y, x), r)
    return table


def rulebook_ref(coords, shape, kernel, stride, padding, subm):
    """-> out_indices (No, 4) int32, out_shape [3], nbr (No, K) int32, inv (Ni, K) int32.
    nbr[o, k] = row of the input site o * stride - pad + k (z-major offsets) or -1; inv[i, k] = row of the output site o with
    o * stride - pad + k == i or -1.  Output sites: the input sites (subm) or every integral in-grid (i + pad - k) / stride,
    ascending in (b, z, y, x)."""
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    kk, st, pd = triple(kernel), triple(stride), triple(padding)
    shape = [int(s) for s in shape]
    offsets = list(itertools.product(range(kk[0]), range(kk[1]), range(kk[2])))       # z-major
    table = site_table(coords, shape)

    def reached(site, off):
        """the output site that input `site` reaches through offset `off`, or None"""
        o = []
        for i, p, k, s, lim in zip(site[1:], pd, off, st, out_shape):
            n = i + p - k
            if n < 0 or n % s or n // s >= lim:
                return None
            o.append(n // s)
        return (site[0],) + tuple(o)

    if subm:
        out_shape, out = list(shape), [tuple(c) for c in coords.tolist()]
    else:
        out_shape = [(s + 2 * p - k) // t + 1 for s, p, k, t in zip(shape, pd, kk, st)]
        sites = set()
        for site in table:
            for off in offsets:
                o = reached(site, off)
                if o is not None:
                    sites.add(o)
        out = sorted(sites)
    nbr = np.full((len(out), len(offsets)), -1, np.int32)
    for r, (b, z, y, x) in enumerate(out):
        for k, (dz, dy, dx) in enumerate(offsets):
            nbr[r, k] = table.get((b, z * st[0] - pd[0] + dz, y * st[1] - pd[1] + dy, x * st[2] - pd[2] + dx), -1)
    otable = {}
    for r, o in enumerate(out):
        otable.setdefault(o, r)
    inv = np.full((coords.shape[0], len(offsets)), -1, np.int32)
    for r, site in enumerate(coords.tolist()):
        for k, off in enumerate(offsets):
            o = reached(tuple(site), off)
            if o is not None:
                inv[r, k] = otable.get(o, -1)
    return np.asarray(out, np.int32).reshape(-1, 4), out_shape, nbr, inv


def linear_keys(coords, shape):
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    return ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]


# ------------------------------------------------------------------------------------------------ value references
def gather_gemm_ref(nbr, x, w, flip=0):
    """out[o] = sum_k x[nbr[o, k]] @ w[K - 1 - k if flip else k] in float64 -> (ref, S, n), each (No, Cout)."""
    nbr, x64, w64 = np.asarray(nbr), np.asarray(x, np.float64), np.asarray(w, np.float64)
    K, cin, cout = w64.shape
    ref, S, n = (np.zeros((nbr.shape[0], cout)) for _ in range(3))
    for k in range(K):
        has = nbr[:, k] >= 0
        wk = w64[K - 1 - k if flip else k]
        ref[has] += x64[nbr[has, k]] @ wk
        S[has] += np.abs(x64[nbr[has, k]]) @ np.abs(wk)
        n[has] += cin
    return ref, S, n


def dgrad_ref(nbr, dout, w, n_in):
    """din[i] = sum over the pairs (o, k) with nbr[o, k] == i of dout[o] @ w[k]^T in float64 -> (ref, S, n), each (n_in, Cin).
    The columns of nbr are injective (one output row per input row and offset), so a fancy-indexed += is exact."""
    nbr, g64, w64 = np.asarray(nbr), np.asarray(dout, np.float64), np.asarray(w, np.float64)
    K, cin, cout = w64.shape
    ref, S, n = (np.zeros((n_in, cin)) for _ in range(3))
    for k in range(K):
        has = nbr[:, k] >= 0
        rows = nbr[has, k]
        assert len(np.unique(rows)) == len(rows), "column %d of the table is not injective" % k
        ref[rows] += g64[has] @ w64[k].T
        S[rows] += np.abs(g64[has]) @ np.abs(w64[k]).T
        n[rows] += cout
    return ref, S, n


def dw_ref(nbr, x, dout):
    """dW[k] = sum_o x[nbr[o, k]]^T dout[o] in float64 -> (ref, S, n), each (K, Cin, Cout); n = P_k, the pairs of offset k."""
    nbr, x64, g64 = np.asarray(nbr), np.asarray(x, np.float64), np.asarray(dout, np.float64)
    K, cin, cout = nbr.shape[1], x64.shape[1], g64.shape[1]
    ref, S, n = (np.zeros((K, cin, cout)) for _ in range(3))
    for k in range(K):
        has = nbr[:, k] >= 0
        a, g = x64[nbr[has, k]], g64[has]
        ref[k], S[k], n[k] = a.T @ g, np.abs(a).T @ np.abs(g), int(has.sum())
    return ref, S, n


def pair_lists(nbr):
    """The definition of Rulebook.pairs(): per offset the (input row, output row) of every output row with a neighbour,
    ascending output row, offsets one after another -> pair_i, pair_o (P) int32, counts (K)."""
    nbr = np.asarray(nbr)
    pi, po = [], []
    for k in range(nbr.shape[1]):
        rows = np.flatnonzero(nbr[:, k] >= 0)
        po.append(rows)
        pi.append(nbr[rows, k])
    cat = (lambda a: np.concatenate(a).astype(np.int32)) if pi else (lambda a: np.zeros(0, np.int32))
    return cat(pi), cat(po), np.array([len(r) for r in po], np.int64)


def wide_range(rng, shape):
    """standard normal rows times a per-CHANNEL scale 10^U(-3, 3): a comparison against the global maximum would miss an error
    in the small channels, the per-element bound does not."""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, (1, shape[1]))).astype(np.float32)


def weights(rng, K, cin, cout):
    return (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ synthetic tables
PLACEMENTS = ("first", "last", "random", "alternate_tiles", "last_block")


def placement_rows(No, placement):
    """The output rows a column may use under `placement`, in the order they are taken."""
    rows = np.arange(No)
    if placement in ("first", "random"):
        return rows
    if placement == "last":
        return rows[::-1]
    if placement == "alternate_tiles":              # every other 64-row tile empty (tiles 1, 3, 5, ...)
        return rows[(rows // 64) % 2 == 0]
    if placement == "last_block":                   # only the last 512-row block of the pair builder
        return rows[rows >= (No - 1) // 512 * 512]
    raise ValueError(placement)


def synthetic_table(No, Ni, K, counts, placement, seed):
    """nbr (No, K) int32: column k has exactly counts[k] valid entries on the rows `placement` selects (one name, or one per
    column); the input rows of a column are distinct rows of [0, Ni) in random order, so a column is injective both ways
    (what the pair kernels require)."""
    rng = np.random.default_rng(seed)
    places = [placement] * K if isinstance(placement, str) else list(placement)
    assert len(counts) == K and len(places) == K
    nbr = np.full((No, K), -1, np.int32)
    for k, (c, pl) in enumerate(zip(counts, places)):
        pool = placement_rows(No, pl)
        if c > len(pool) or c > Ni:
            raise ValueError("column %d: %d entries do not fit placement %s" % (k, c, pl))
        rows = rng.choice(pool, c, replace=False) if pl == "random" else pool[:c]
        nbr[rows, k] = rng.permutation(Ni)[:c]
    return nbr


# Main table: 8 200 rows = 16 full 512-row blocks of the pair builder + 8 rows = 8 rows past the 8 192-row chunk of the table
# weight gradient; per-offset pair counts at, one below and one above the 64-pair tile (x1, x2, x3), the 4 096-pair item, and
# the whole table.
MAIN_ROWS, MAIN_K = 8200, 27
COUNT_VALUES = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4095, 4096, 4097, 8200)


def main_table():
    rng = np.random.default_rng(20)
    counts = list(COUNT_VALUES) + [int(c) for c in rng.choice(COUNT_VALUES[:-1], MAIN_K - len(COUNT_VALUES))]
    counts = [counts[i] for i in rng.permutation(MAIN_K)]
    places, small = [], 0
    for k, c in enumerate(counts):
        pl = PLACEMENTS[k % 4]
        if 0 < c <= MAIN_ROWS - 8192 and small < 2:         # the 8 rows of the last 512-row block hold only the smallest columns
            pl, small = "last_block", small + 1
        places.append(pl if c <= len(placement_rows(MAIN_ROWS, pl)) else "random")
    return synthetic_table(MAIN_ROWS, MAIN_ROWS, MAIN_K, counts, places, 21), counts, places


SMALL_K = (1, 2, 3, 8)
SMALL_ROWS = 193


def small_table(K):
    """(193, K): a full, a nearly empty and ragged columns; K = 1 is one full column."""
    counts = [193, 0, 64, 1, 65, 127, 192, 63][:K]
    return synthetic_table(SMALL_ROWS, SMALL_ROWS, K, counts, "random", 30 + K)


def builder_tables():
    """name -> nbr for the pair-list builder: the main table, the small-K tables, rows only in the last (ragged) 512-row block,
    and every other 64-row tile empty on one block + 1 row."""
    out = {"main": main_table()[0]}
    for K in SMALL_K:
        out["small_k%d" % K] = small_table(K)
    out["last_block"] = synthetic_table(1500, 1500, 3, [476, 0, 65], "last_block", 40)
    out["alternate_tiles"] = synthetic_table(513, 600, 5, [257, 64, 0, 1, 256], "alternate_tiles", 41)
    out["one_row"] = synthetic_table(1, 1, 2, [1, 0], "first", 42)
    return out


# ------------------------------------------------------------------------------------------------ row counts / channel plans
# LDS kernel: 64 rows per workgroup; register kernel: 128 per workgroup, 32 per wave; pair builder: 512-row blocks
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
ROWS_PLANS = ((16, 16), (33, 40))
ROWS_GRID = (5, 12, 24)                # 1 440 cells


def rows_case(n):
    """A submanifold k3 rulebook input with exactly n sites on ROWS_GRID, rows in random order."""
    rng = np.random.default_rng(100 + n)
    cells = rng.choice(int(np.prod(ROWS_GRID)), n, replace=False)
    z, y, x = np.unravel_index(cells, ROWS_GRID)
    return np.stack([np.zeros(n, np.int64), z, y, x], 1).astype(np.int32)


PLAN_ROWS = 193
PLANS_REGISTER_FLOAT4 = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 32), (64, 64), (128, 64), (16, 4))
PLANS_REGISTER_SCALAR = ((9, 20), (16, 33), (17, 64), (33, 40), (100, 33), (24, 40))
PLANS_LDS = ((1, 1), (3, 5), (4, 16), (5, 128), (64, 96), (64, 128), (128, 16))
PLANS_LDS_BIG = ((128, 128),)                       # 105 KB of dynamic LDS at K = 27
PLANS = PLANS_REGISTER_FLOAT4 + PLANS_REGISTER_SCALAR + PLANS_LDS + PLANS_LDS_BIG
PLANS_SMALL_K = ((16, 16), (33, 40), (5, 128))      # register float4, register scalar, LDS

DW_PAIR_PLANS = ((1, 1), (2, 128), (128, 2), (4, 16), (16, 16), (16, 32), (32, 64), (64, 64), (64, 128), (128, 128))
DW_TABLE_PLANS = ((3, 5), (24, 40), (33, 70), (100, 100), (128, 128))

PAIR_ITEM_SIZES = (1, 64, 65, 128, 129, 192, 193, 4096)       # ntiles 1, 1, 2, 2, 3, 3, 4, 64
PAIR_GEMM_PLANS = ((4, 16), (16, 4), (64, 64), (128, 128), (16, 33))


def pair_item_table(p):
    """(p + 9, 2) over p + 7 input rows: offset 0 has p pairs on random rows; offset 1 has min(p, 65) pairs on output rows and input
    rows that offset 0 uses as well (a read-modify-write of the same destinations), so 9 output and 7 input rows are in no pair."""
    col0 = synthetic_table(p + 9, p + 7, 1, [p], "random", 500 + p)[:, 0]
    rows = np.random.default_rng(p).permutation(np.flatnonzero(col0 >= 0))[:min(p, 65)]
    col1 = np.full_like(col0, -1)
    col1[rows] = np.roll(col0[rows], 1)
    return np.stack([col0, col1], 1)


def register_kernel_takes(cin, cout):
    """The channel table of mgar_spconv_gather_gemm, restated: (takes the register kernel, on its float4 path)."""
    cinp = 4 if cin <= 4 else 16 if cin <= 16 else 32 if cin <= 32 else 64 if cin <= 64 else 128
    ncb = (cout + 31) // 32
    return (cinp, ncb) in ((16, 1), (32, 1), (32, 2), (64, 1), (64, 2), (128, 2), (16, 2)), cin == cinp


# ------------------------------------------------------------------------------------------------ geometry cases
GEOMETRIES = {   # name: (subm, kernel, stride, padding) -- the four layer geometries of VoxelBackBone8x and k2 s2 p0
    "subm_k3": (True, 3, 1, 1),
    "k3_s2_p1": (False, 3, 2, 1),
    "k3_s2_p011": (False, 3, 2, (0, 1, 1)),
    "k311_s211_p0": (False, (3, 1, 1), (2, 1, 1), 0),
    "k2_s2_p0": (False, 2, 2, 0),
}
PRODUCTION_SHAPE, PRODUCTION_BATCH = (41, 1600, 1408), 32
PRODUCTION_SMALL_SHAPE = (41, 16, 16)       # the same distances to every face; shifts (0, 1584, 1392): multiples of the stride


def _shuffled(rng, rows):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    return rows[rng.permutation(len(rows))].astype(np.int32)


def _full(batch, shape):
    return [(b, z, y, x) for b in range(batch) for z in range(shape[0]) for y in range(shape[1]) for x in range(shape[2])]


def production_clusters():
    """~300 sites: one cluster in the low corner of sample 0, one in the high corner of sample 31 (keys above 2^31).
    -> coords at the shipped grid and the same sites translated into PRODUCTION_SMALL_SHAPE, batch 2."""
    rng = np.random.default_rng(7)
    Z, Y, X = PRODUCTION_SHAPE
    lo = np.stack(np.unravel_index(rng.choice(6 * 7 * 7, 150, replace=False), (6, 7, 7)), 1)
    hi = np.stack(np.unravel_index(rng.choice(5 * 7 * 7, 150, replace=False), (5, 7, 7)), 1)
    big = np.concatenate([np.concatenate([np.zeros((150, 1), np.int64), lo], 1),
                          np.concatenate([np.full((150, 1), PRODUCTION_BATCH - 1), hi + [Z - 5, Y - 7, X - 7]], 1)])
    perm = rng.permutation(300)
    small = big.copy()
    small[150:] -= [PRODUCTION_BATCH - 2, 0, Y - PRODUCTION_SMALL_SHAPE[1], X - PRODUCTION_SMALL_SHAPE[2]]
    return big[perm].astype(np.int32), small[perm].astype(np.int32)


def geometry_inputs():
    """name -> (coords (N, 4) int32, shape, batch): the inputs of the geometry cases."""
    rng = np.random.default_rng(3)
    out = {}
    # every boundary condition (6 faces, 12 edges, 8 corners), interior rows with all 27 neighbours, odd extents under stride 2
    out["faces"] = (_shuffled(rng, _full(2, (5, 6, 7))), (5, 6, 7), 2)
    for shape in ((1, 1, 40), (1, 9, 1), (41, 1, 1)):                               # grids one cell thick
        cells = [c for c in _full(2, shape) if rng.random() < 0.6]
        out["thin_%dx%dx%d" % shape] = (_shuffled(rng, cells), shape, 2)
    # sites >= 3 cells apart: a submanifold convolution uses its centre tap only
    iso = [(b, z, y, x) for b in range(2) for z in (0, 3, 6) for y in (0, 3, 6, 9) for x in (1, 4, 7, 10) if rng.random() < 0.7]
    out["isolated"] = (_shuffled(rng, iso), (7, 10, 11), 2)
    # samples 1 and 3 empty; the last cell of sample 0 and the first of sample 2 are neighbours in the linear key only
    gaps = [(0, 2, 3, 4), (0, 2, 3, 3), (0, 2, 2, 4), (0, 1, 3, 4), (0, 1, 2, 3), (0, 0, 0, 0),
            (2, 0, 0, 0), (2, 0, 0, 1), (2, 0, 1, 0), (2, 1, 0, 0), (2, 1, 1, 1), (2, 2, 3, 4)]
    out["batch_gaps"] = (_shuffled(rng, gaps), (3, 4, 5), 4)
    # Z = 6 under k (3, 1, 1) s (2, 1, 1) p 0: output planes 0 and 1 read z 0..4, the plane z = 5 reaches no output
    plane = [(b, z, y, x) for b in range(2) for z in range(6) for y in range(4) for x in range(5) if rng.random() < (0.8 if z == 5 else 0.4)]
    out["dropped_plane"] = (_shuffled(rng, plane), (6, 4, 5), 2)
    out["dropped_plane_only"] = (_shuffled(rng, [c for c in plane if c[1] == 5]), (6, 4, 5), 2)       # No = 0 there
    out["empty"] = (np.zeros((0, 4), np.int32), (5, 6, 7), 2)
    out["production_keys"] = (production_clusters()[0], PRODUCTION_SHAPE, PRODUCTION_BATCH)
    return out


def geometry_cases():
    """[(case, geometry, coords, shape, batch, subm, kernel, stride, padding)] wherever the geometry applies: an output grid
    with an extent below 1 (a one-cell-thick axis under an unpadded k 3 / k 2) is outside the layer's definition."""
    out = []
    for case, (coords, shape, batch) in geometry_inputs().items():
        for gname, (subm, kernel, stride, padding) in GEOMETRIES.items():
            oshape = [(s + 2 * p - k) // t + 1 for s, p, k, t in zip(shape, triple(padding), triple(kernel), triple(stride))]
            if min(oshape) >= 1:
                out.append((case, gname, coords, shape, batch, subm, kernel, stride, padding))
    return out


GEOMETRY_IDS = ["%s-%s" % (c[0], c[1]) for c in geometry_cases()]
CONV_CHANNELS = ((4, 16), (5, 7))       # powers of two (pair-list kernels where switched on) and not (table kernels)


def conv_tensors(case, gname, n_in, K, cin, cout):
    """Seeded features (n_in, cin), weight (K, cin, cout) of a whole-op case; the cotangent is drawn by conv_cotangent once the
    number of output sites is known."""
    rng = np.random.default_rng(abs(hash((len(case), len(gname), n_in, K, cin, cout))) % 2 ** 31)
    return wide_range(rng, (n_in, cin)), weights(rng, K, cin, cout)


def conv_cotangent(n_out, cout):
    return wide_range(np.random.default_rng(900 + n_out + cout), (n_out, cout))


# ------------------------------------------------------------------------------------------------ hash cases
HASH_SHAPE, HASH_BATCH = (6, 7, 8), 3
HASH_N = (0, 1, 8, 9, 512, 513)         # 8 and 512: load exactly 0.5 (capacity 16 / 1 024); 9 and 513: the next capacity


def hash_queries(rng, coords):
    Z, Y, X = HASH_SHAPE
    q = [c for c in np.asarray(coords).reshape(-1, 4).tolist()]                                       # every build row
    q += [[b, z, y, x] for b, z, y, x in zip(rng.integers(0, HASH_BATCH + 1, 200), rng.integers(0, Z, 200), rng.integers(0, Y, 200),
                                             rng.integers(0, X, 200))]                                 # present or absent; b = batch: absent
    q += [[1, -1, 2, 3], [1, Z, 2, 3], [1, 2, -1, 3], [1, 2, Y, 3], [1, 2, 3, -1], [1, 2, 3, X]]      # outside each of the six faces
    q += [[0, -1, Y - 1, X - 1], [0, 0, -1, X], [2, Z - 1, Y - 1, X], [1, 0, Y, 0]]                   # keys that would alias a neighbour cell
    q += [[-1, 0, 0, 0], [-1, 2, 3, 4], [-2, Z - 1, Y - 1, X - 1]]                                    # b < 0
    return np.asarray(q, np.int32).reshape(-1, 4)


def hash_cases():
    """name -> (build coords, query coords, expected rows from the dict)."""
    out = {}
    cells = np.asarray(_full(HASH_BATCH, HASH_SHAPE), np.int64)
    for n in HASH_N:
        rng = np.random.default_rng(60 + n)
        out["n%d" % n] = cells[rng.choice(len(cells), n, replace=False)].astype(np.int32).reshape(-1, 4)
    rng = np.random.default_rng(59)
    dup = cells[rng.choice(len(cells), 40, replace=False)].astype(np.int32)
    dup[[5, 17, 39]] = dup[[30, 2, 0]]                   # duplicated coordinates: the smallest row wins (rows 5, 2 and 0)
    dup[20] = dup[21] = dup[3]
    out["duplicates"] = dup
    bad = cells[rng.choice(len(cells), 40, replace=False)].astype(np.int32)
    bad[[0, 7, 13, 21, 30, 39], [1, 1, 2, 2, 3, 3]] = [-1, HASH_SHAPE[0], -1, HASH_SHAPE[1], -1, HASH_SHAPE[2]]
    bad[[4, 25], 0] = [-1, -3]                            # negative batch index at build time: not inserted
    out["out_of_grid"] = bad
    res = {}
    for name, coords in out.items():
        rng = np.random.default_rng(len(name) + len(coords))
        q = hash_queries(rng, coords)
        table = site_table(coords, HASH_SHAPE)
        res[name] = (coords, q, np.array([table.get(tuple(c), -1) if c[0] >= 0 else -1 for c in q.tolist()], np.int32))
    return res
