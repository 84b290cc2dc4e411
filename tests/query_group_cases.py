"""Seeded inputs of the op-level tests of csrc/query_group.hip, shared by tests/test_query_group_cpu.py -- which checks,
with no kernel involved, the float64 references (torch_refs.py) against the C oracle's op chain and that the device
bounds are satisfiable -- and tests/test_query_group_gpu.py.

The neighbour indices are built with numpy, duplicates, empty balls and garbage slots put in by hand: what is under test
is the grouping, not the ball query.  Every case names the code path it is there for.  All arrays are numpy, fp32 / int32."""
import numpy as np

# ------------------------------------------------------------------------------------------------ batch forward
# qg_batch_fwd_kernel: 256 columns per block (cols = npoints * nsample: 1, 255 / 257 around one block, 1 875 = 375 x 5 with
# a partial last block), QG_CCHUNK = 8 channels per blockIdx.y (c = 0 no feature block, 1 / 7 a tail only, 8 exact, 9 / 17
# a tail after full chunks), b on blockIdx.z.
BATCH_FWD_CASES = {
    # id: b, c, npoints, nsample, n
    "c0_cols1_b1": (1, 0, 1, 1, 4),
    "c8_cols1_b3": (3, 8, 1, 1, 7),
    "c1_cols255_b3": (3, 1, 51, 5, 40),
    "c9_cols255_b1": (1, 9, 51, 5, 33),
    "c7_cols257_b1": (1, 7, 257, 1, 300),
    "c17_cols257_b3": (3, 17, 257, 1, 64),
    "c8_cols1875_b3": (3, 8, 375, 5, 500),
    "c17_cols1875_b1": (1, 17, 375, 5, 2000),
}


def batch_fwd_case(name):
    b, c, m, ns, n = BATCH_FWD_CASES[name]
    rng = np.random.default_rng(1000 + sorted(BATCH_FWD_CASES).index(name))
    idx = rng.integers(0, n, (b, m, ns)).astype(np.int32)
    if ns > 1:
        idx[:, :, 1] = 3 % n                       # one slot column: the same point for every query
        idx[:, m // 2, :] = idx[:, m // 2, :1]     # one query: the same point in every slot (first-hit padding)
    idx[:, 0, 0] = 0                               # the first and the last point of the cloud
    idx[:, -1, -1] = n - 1
    if m * ns == 1:
        idx[0] = 0                                 # one column per sample: sample 0 takes point 0, the others point n - 1
    return dict(b=b, c=c, m=m, ns=ns, n=n, idx=idx,
                xyz=rng.uniform(-4, 4, (b, n, 3)).astype(np.float32),
                new_xyz=rng.uniform(-4, 4, (b, m, 3)).astype(np.float32),
                feats=rng.standard_normal((b, c, n)).astype(np.float32),
                wx=rng.standard_normal((c, 3)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ batch backward
# qg_batch_bwd: n <= 36 864 takes qg_batch_bwd_lds_kernel (one int64 window up to n = 18 432, two above), larger n the
# float-atomic qg_batch_bwd_atomic_kernel; cols >= 4 096 launches 1 024 threads, fewer 256; cols % 4 != 0 takes the scalar
# loads (and the gradient rows then start off 16-byte boundaries).
BWD_N = (18432, 18433, 36864, 36865, 40000)
BWD_COLS = {512: (16, 32), 4096: (128, 32), 1875: (375, 5)}
BWD_B, BWD_C = 2, 3
LDS_MAX_N, LDS_WINDOW = 36864, 18432


def batch_bwd_case(n, cols, single_cell=None):
    """single_cell: every column of every sample points at that one cell (k = cols)."""
    m, ns = BWD_COLS[cols]
    rng = np.random.default_rng(n * 7 + cols)
    # half of the columns fall on 16 hot cells (many contributions each) that sit on the ends of the row and on both sides
    # of the window cuts; the other half is spread over the row
    hot = np.unique(np.clip(np.concatenate([[0, 1, n - 2, n - 1, LDS_WINDOW - 1, LDS_WINDOW, LDS_MAX_N - 1, LDS_MAX_N],
                                            rng.integers(0, n, 8)]), 0, n - 1))
    idx = np.where(rng.random((BWD_B, cols)) < 0.5, hot[rng.integers(0, len(hot), (BWD_B, cols))], rng.integers(0, n, (BWD_B, cols)))
    if single_cell is not None:
        idx[:] = single_cell
    shape = (BWD_B, 3 + BWD_C, cols)
    g = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)
    return dict(b=BWD_B, c=BWD_C, n=n, m=m, ns=ns, cols=cols, idx=idx.astype(np.int32), g=g)


# ------------------------------------------------------------------------------------------------ stack
# qg_stack_{fwd,bwd}_kernel: 128 columns per workgroup, 32 channels per LDS pass.  nsample = 16: a tile is 8 queries, so
# with NEW_CNT the first tile covers samples 0, 2 and 3 (sample 1 has no query): one segment search cannot serve it.
STACK_NS = 16
STACK_XYZ_CNT = (40, 7, 0, 300, 9)          # sample 2 has no point: its two queries can only be empty balls
STACK_NEW_CNT = {"ragged": (3, 0, 2, 150, 1),     # M * ns = 2 496 = 19.5 tiles
                 "tiles": (3, 0, 2, 150, 5)}      # M * ns = 2 560 = 20 tiles (what _fwd_stats needs)
STACK_C = (0, 1, 31, 32, 33, 64, 65)
STACK_LD_PAD, STACK_BASE_OFFSET = 5, 3      # zf_ld = C + 5; the base pointer 3 floats into its buffer (not 16-byte aligned)
STACK_EMPTY_TILE = 5                        # layout "tiles": queries 40..47 are all empty


STACK_DENSE_XYZ_CNT = (40, 7, 11, 300, 9)


def stack_case(layout, C, shift=0.0, scale=1.0, dense=False):
    """feats (N, C) = shift + scale * standard normal.  dense: every sample has points and no ball is empty, so with
    shift 100 and scale 0.1 every tile of y has |mean| >> std (wx is scaled down with the features: wx . rel stays small);
    an empty ball in a tile would put zeros next to the hundreds and the variance digits would stop mattering."""
    xyz_cnt, new_cnt = np.array(STACK_DENSE_XYZ_CNT if dense else STACK_XYZ_CNT, np.int32), np.array(STACK_NEW_CNT[layout], np.int32)
    N, M, ns = int(xyz_cnt.sum()), int(new_cnt.sum()), STACK_NS
    rng = np.random.default_rng(50 + C + (1000 if layout == "tiles" else 0))
    sample = np.repeat(np.arange(len(new_cnt)), new_cnt)
    q_start = np.concatenate([[0], np.cumsum(new_cnt)[:-1]])
    idx = np.zeros((M, ns), np.int32)
    empty = np.arange(M) % 7 == 0                                          # every 7th query
    empty[q_start[3]] = empty[q_start[3] + new_cnt[3] - 1] = True          # the first and the last query of sample 3
    empty[xyz_cnt[sample] == 0] = True
    if layout == "tiles":
        empty[STACK_EMPTY_TILE * 8:(STACK_EMPTY_TILE + 1) * 8] = True
    if dense:
        empty[:] = False
    for q in range(M):
        cnt = int(xyz_cnt[sample[q]])
        if empty[q]:
            # garbage in slots 1..: non-zero, and small enough to stay inside the arrays if a kernel wrongly followed it
            idx[q] = rng.integers(1, min(xyz_cnt[-1], 9), ns)
            idx[q, 0] = -1
            continue
        found = rng.integers(1, ns + 1)
        idx[q, :found] = rng.integers(0, cnt, found)
        idx[q, found:] = idx[q, 0]                                         # first-hit padding: duplicates
    live = np.flatnonzero(~empty & (sample == 3))[1:]
    idx[live[0], 0], idx[live[1], -1] = 0, xyz_cnt[3] - 1                  # first and last point of a sample
    idx[live[1], :-1] = 0
    shape = (3 + C, M * ns)
    return dict(B=len(new_cnt), N=N, M=M, ns=ns, C=C, xyz_cnt=xyz_cnt, new_cnt=new_cnt, idx=idx, empty=empty,
                xyz=rng.uniform(-4, 4, (N, 3)).astype(np.float32),
                new_xyz=rng.uniform(-4, 4, (M, 3)).astype(np.float32),
                feats=(shift + scale * rng.standard_normal((N, C))).astype(np.float32),
                wx=(rng.standard_normal((C, 3)) * (0.1 * scale if dense else 1.0)).astype(np.float32),
                g=(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32))
