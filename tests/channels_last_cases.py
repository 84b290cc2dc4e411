"""Seeded inputs of the op-level tests of csrc/channels_last.hpp (channels-last / row-major BatchNorm, NCDHW -> NDHWC apply,
channels-last max pooling) and csrc/maxpool3d.hip, shared by tests/test_channels_last_cpu.py -- which checks, with no kernel,
the float64 references and the bounds of torch_refs.py -- and tests/test_channels_last_ops_gpu.py, test_maxpool3d_gpu.py,
test_nonfinite_forward_gpu.py.

Every case names the edge it is there for; the shapes are the smallest that reach it, read off the constants of
channels_last.hpp: CL_THREADS = 256 (a thread = one float4 channel group x one row lane, rpar = 256 // (C / 4) row lanes,
256 - rpar * (C / 4) idle threads), cl_chunk_rows (>= 256 rows, about 2 048 workgroups, capped at R), the 64 x 64 transpose
tile, C % 4 == 0, C <= 1024, S * C <= 65535; and of maxpool3d.hip: the quad kernels need kw == 3, W % 4 == 0, Wo % 4 == 0,
kt <= 3, NC <= 65535 (stride 2 also W >= 8), everything else takes the one-thread-per-output kernel.
All arrays are numpy fp32.  Channels-last tensors are (S, R, C): S samples of R rows; mean / invstd of the apply and backward
cases are INPUTS of those entry points (float64 statistics of the first draw of x, rounded to fp32); x is then moved off the
ReLU threshold with bn_act_cases.off_threshold."""
import itertools

import numpy as np

import bn_act_cases as BC
from bn_act_cases import EPS, GROUP_MEANS, GROUP_STDS, MOMENTA, _seed   # noqa: F401

# ------------------------------------------------------------------------------------------------ statistics
STATS_CASES = {
    # id: (S, R, C, per_sample, mean, std, what)
    "c4_256_row_lanes": (1, 300, 4, 0, 0.7, 2.0, "ng = 1, rpar = 256: every thread a row lane; chunk 1 holds 44 rows"),
    "c24_rpar42_4_idle": (1, 300, 24, 0, 0.7, 2.0, "ng = 6, rpar = 42: threads 252..255 idle"),
    "c516_rpar1_127_idle": (1, 300, 516, 0, 0.7, 2.0, "ng = 129, rpar = 1: threads 129..255 idle"),
    "c1024_no_row_lanes": (1, 300, 1024, 0, 0.7, 2.0, "ng = 256: every thread a column group"),
    "one_row": (1, 1, 8, 0, 0.7, 2.0, "R = 1: var = 0 exactly, invstd = fp32(1 / sqrt(eps)), no unbiased correction"),
    "r7_c16_fewer_rows_than_lanes": (1, 7, 16, 0, 0.7, 2.0, "7 rows, 64 row lanes"),
    "r257_last_chunk_of_1": (1, 257, 8, 0, 0.7, 2.0, "chunk 1 is one row: its M2 is exactly 0"),
    "chunk_293": (1, 600000, 4, 0, 0.7, 2.0, "chunk 293 > 256, 2 048 chunks, the last holds 229 rows; 9.6 MB"),
    "per_sample_s3": (3, 300, 8, 1, None, None, "S = 3 far-apart samples, chunk 1 ragged (44 rows); updates in sample order"),
    "s3_chunks_cross_samples": (3, 300, 8, 0, 0.7, 2.0, "not per-sample: 900 rows, chunks start at 256, 512, 768"),
    "cancellation_mean1e4": (1, 300, 8, 0, 1e4, 1.0, "|mean| = 1e4 std: the pivot keeps the variance digits"),
    # One chunk of 256 rows whose pivot row IS the outlier: every x - p is about -1e6 and s = sum (x - p) about -2.55e8.
    # bn_merge_bounds' own `low > 0` holds (dvar / var = 6e-3, measured in test_channels_last_cpu.py); the invstd bound is
    # 3.0e-3 of invstd, some 4 000 times the 7.2e-7 of bn_act.hip's outlier_in_pivot: there the pivot is the mean of 256
    # elements (1e6 / 256 away from the bulk) and a lane adds 16 terms before a tree, here the pivot is the single row itself
    # (1e6 away from the bulk) under a chain of 130 additions, and |s| |ds| / nk grows with the square of that distance.
    "outlier_in_pivot_row": (1, 256, 8, 0, 0.0, 1.0, "one chunk, 1e6 in its first row = the pivot"),
}


def stats_case(name):
    S, R, C, per, mean, std, _ = STATS_CASES[name]
    rng = np.random.default_rng(_seed(name))
    x = rng.standard_normal((S, R, C), dtype=np.float32)
    if per:
        for s in range(S):
            x[s] = GROUP_MEANS[s] + GROUP_STDS[s] * x[s]
    else:
        x = (mean + std * x).astype(np.float32)
    if name == "outlier_in_pivot_row":
        x[0, 0, :] = 1e6
    return dict(S=S, R=R, C=C, per_sample=per, x=x, running_mean=rng.standard_normal(C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C).astype(np.float32), nbt=7)


# ------------------------------------------------------------------------------------------------ apply
APPLY_C = (4, 24, 516, 1024)
APPLY_AFFINE = BC.APPLY_AFFINE
APPLY_PAD = 8                                   # ldy = C + 8: the Inception concatenation's column slice
APPLY_SHAPES = {"s3_r5": (3, 5), "total_257": (1, 257)}    # total_257 at C = 4: rows * (C / 4) one past a multiple of 256


def to_bcp(x):
    """(S, R, C) rows -> (S, C, R), the (B, C, P) view torch_refs' bn_apply_ref / bn_bwd_ref take."""
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 1))


to_rows = to_bcp          # (S, C, R) -> (S, R, C): the transpose is its own inverse; the second name says which way a call goes


def apply_case(S, R, C, which, per_sample, relu=True, seed=0):
    """x (S, R, C); mean / invstd (C,) or (S * C,) with per-sample statistics; gamma has a negative entry and, with "both",
    a zero entry.  relu=False keeps the near-zero values (x of row 0 is the mean: the pre-activation is exactly beta or 0)."""
    rng = np.random.default_rng(S * 1000003 + R * 1009 + C * 7 + APPLY_AFFINE.index(which) * 2 + per_sample + seed)
    xc = (0.7 + 2.0 * rng.standard_normal((S, C, R), dtype=np.float32)).astype(np.float32)
    m, v = BC.stats_of(xc.reshape(1, S * C, R) if per_sample else xc)
    mean32, invstd32 = m.astype(np.float32), ((v + EPS) ** -0.5).astype(np.float32)
    gamma, beta = BC.affine(C, which, rng)
    if relu:
        BC.off_threshold(xc, mean32, invstd32, gamma, beta, bool(per_sample))
    else:
        xc[:, :, 0] = mean32.reshape(S, C) if per_sample else mean32[None, :]
    return dict(S=S, R=R, C=C, x=to_rows(xc), xc=xc, mean=mean32, invstd=invstd32, gamma=gamma, beta=beta)


# ------------------------------------------------------------------------------------------------ NCDHW -> NDHWC
TO_CL_R, TO_CL_C, TO_CL_S = (1, 63, 64, 65), (1, 3, 64, 65), 2      # around the 64 x 64 tile; this entry has no C % 4 rule


def to_cl_case(R, C, per_sample, relu=True):
    """xc (S, C, R) is the entry's NCDHW input, x (S, R, C) what its output is laid out like."""
    return apply_case(TO_CL_S, R, C, "both", per_sample, relu, seed=77)


# ------------------------------------------------------------------------------------------------ row-major backward
BWD_CASES = {
    # id: (rows, C)
    "one_row_c8": (1, 8), "r7_c24_rpar42": (7, 24), "r257_c4_last_chunk_of_1": (257, 4), "r257_c516_rpar1": (257, 516),
    "r300_c1024": (300, 1024), "chunk_293_c4": (600000, 4),
}


def bwd_case(name, relu, which="both"):
    """x, dy (rows, C) row-major; xc, dyc their (1, C, rows) views for the references."""
    rows, C = BWD_CASES[name]
    k = BC.bwd_case(1, C, rows, relu, which, seed=31)
    return dict(rows=rows, C=C, xc=k["x"], dyc=k["dy"], x=to_rows(k["x"])[0], dy=to_rows(k["dy"])[0], mean=k["mean"],
                invstd=k["invstd"], gamma=k["gamma"], beta=k["beta"])


# ------------------------------------------------------------------------------------------------ rejections
# (S, R, C) that mgar_bn_cl_train_stats and mgar_bn_cl_act_fwd return MGAR_EINVAL for before any launch (the ldy and alignment
# rejections are written out in the two test files)
CL_REJECTED_SHAPES = {"c_not_multiple_of_4": (1, 8, 6), "c_1028": (1, 8, 1028)}
S_TIMES_C_TOO_LARGE = (64, 2, 1024)          # S * C = 65 536 > 65 535 with per-sample statistics

# ------------------------------------------------------------------------------------------------ pooling
I3D_GEOMETRIES = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)))


def _pool_cases():
    cases = {}

    def add(route, NC, T, H, W, k, s, tag=""):
        cases["%s_nc%d_%dx%dx%d_k%d%d%d_s%d%d%d%s" % ((route, NC, T, H, W) + tuple(k) + tuple(s) + (tag,))] = \
            dict(route=route, NC=NC, T=T, H=H, W=W, k=tuple(k), s=tuple(s), negative=tag == "_negative")
    # stride-1 quad kernel: W = 4 is one quad that is both the left and the right edge; H = 1; every T up to one past the
    # three-slice register window; every kt <= 3 at both strides in t
    for W, T in itertools.product((4, 8), (1, 2, 3, 4)):
        for kt, st in itertools.product((1, 2, 3), (1, 2)):
            add("quad1", 3, T, 1 if (T + kt + st) % 2 else 3, W, (kt, 3, 3), (st, 1, 1))
    # stride-2 quad kernel: W = 8 is one quad; T odd (front padding 1 in t) and even (0); kh 1 and 3
    for W, T, kh in itertools.product((8, 16), (3, 4), (1, 3)):
        add("quad2", 3, T, 5 if T == 3 else 6, W, (3, kh, 3), (2, 2, 2))
    # one-thread-per-output kernel: Wo % 4 != 0, kt = 4, k = s = 2, and the NC <= 65535 gate of the quad kernels
    add("scalar", 3, 3, 4, 6, (3, 3, 3), (2, 2, 2))
    add("scalar", 3, 4, 5, 12, (3, 3, 3), (2, 2, 2))
    add("scalar", 3, 5, 3, 8, (4, 3, 3), (1, 1, 1))
    add("scalar", 3, 4, 5, 6, (2, 2, 2), (2, 2, 2))
    add("scalar", 65536, 1, 1, 4, (3, 3, 3), (1, 1, 1))
    # all-negative input: "valid" differs from "same" wherever the window leaves the input
    add("quad1", 2, 3, 4, 8, (3, 3, 3), (1, 1, 1), "_negative")
    add("quad2", 2, 3, 4, 8, (3, 3, 3), (2, 2, 2), "_negative")
    add("scalar", 2, 3, 4, 6, (3, 3, 3), (2, 2, 2), "_negative")
    return cases


POOL_CASES = _pool_cases()


def pool_route(NC, T, H, W, k, s):
    """Which kernel maxpool3d_same_fwd_impl launches: its dispatch condition restated."""
    import torch_refs as R
    pw, Wo = R.same_pads(W, k[2], s[2])[0], -(-W // s[2])
    vec1 = k[2] == 3 and s[2] == 1 and pw == 1
    vec2 = k[2] == 3 and s[2] == 2 and pw == 0 and W % 2 == 0
    if (vec1 or vec2) and k[0] <= 3 and W % 4 == 0 and Wo % 4 == 0 and NC <= 65535 and (not vec2 or W >= 8):
        return "quad1" if vec1 else "quad2"
    return "scalar"


def pool_input(shape, seed, negative=False):
    """randn - 0.5, so that the zero padding wins at many borders; negative: every element < 0."""
    x = np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) - np.float32(0.5)
    return (-np.abs(x) - np.float32(0.1)).astype(np.float32) if negative else x


def pool_case(name):
    c = POOL_CASES[name]
    return dict(c, x=pool_input((c["NC"], c["T"], c["H"], c["W"]), _seed(name), c["negative"]))


POOL_CL_C = (4, 8, 24)
POOL_CL_THW = ((1, 1, 1), (2, 3, 5), (3, 4, 4))
POOL_CL_GEOMETRIES = I3D_GEOMETRIES + (((2, 2, 2), (2, 2, 2)),)
POOL_CL_N = 2


def pool_cl_case(C, thw, k, s):
    """x (N, C, T, H, W) for the reference; the entry reads np.moveaxis(x, 1, -1)."""
    x = pool_input((POOL_CL_N, C) + tuple(thw), C * 1000 + thw[0] * 100 + thw[1] * 10 + thw[2] + k[0] * 7 + s[0])
    return dict(N=POOL_CL_N, C=C, T=thw[0], H=thw[1], W=thw[2], k=tuple(k), s=tuple(s), x=x,
                x_cl=np.ascontiguousarray(np.moveaxis(x, 1, -1)))


# where a NaN goes in the non-finite pool tests: (case, (t, h, w), what it covers)
POOL_NAN_SITES = (
    ("quad1_nc3_4x3x8_k333_s111", (1, 1, 5), "interior"),
    ("quad1_nc3_4x3x8_k333_s111", (0, 0, 0), "corner: the window also holds padding"),
    ("quad1_nc3_4x3x8_k333_s111", (3, 2, 7), "far corner"),
    ("quad1_nc3_4x3x8_k333_s111", (2, 1, 3), "w = 3: the lft load of quad 1"),
    ("quad1_nc3_4x3x8_k333_s111", (2, 1, 4), "w = 4: the rgt load of quad 0"),
    ("quad1_nc3_4x3x8_k333_s111", (0, 1, 2), "slice t - 2 of the window emitted at t = 2: the p0 register"),
    ("quad1_nc3_1x1x4_k133_s111", (0, 0, 0), "one quad, left edge sentinel"),
    ("quad1_nc3_1x1x4_k133_s111", (0, 0, 3), "one quad, right edge sentinel"),
    ("quad2_nc3_4x6x16_k333_s222", (1, 2, 8), "w = 8: the rgt load of quad 0"),
    ("quad2_nc3_4x6x16_k333_s222", (2, 3, 7), "interior, u.w"),
    ("quad2_nc3_4x6x16_k333_s222", (3, 5, 15), "far corner: rgt is the sentinel, t and h windows clipped"),
    ("quad2_nc3_3x5x8_k333_s222", (0, 0, 0), "corner, front padding 1 in t"),
    ("quad2_nc3_4x6x16_k333_s222", (0, 2, 3), "slice t - 2 of the window emitted at t = 2: the p0 register"),
    ("scalar_nc3_3x4x6_k333_s222", (1, 2, 3), "interior"),
    ("scalar_nc3_3x4x6_k333_s222", (0, 0, 0), "corner"),
    ("scalar_nc3_5x3x8_k433_s111", (4, 2, 7), "far corner, kt = 4"),
)
