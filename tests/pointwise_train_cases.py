"""Seeded inputs, float64 references, rounding-count bounds and the restated launch geometry of the op-level tests of the
fp32 TRAINING kernels of the shared MLPs: csrc/pointwise_fwd.hip (forward, transposed forward = data gradient, STATS epilogue,
GRAD operand mode), csrc/pointwise_dw.hip (plain, _act, pair mode, GRAD instances, the partial reduce) and csrc/rowmajor_dw.hip.
Shared by tests/test_pointwise_train_cpu.py -- which checks, with no kernel, that the references are torch's autograd of the
same expressions, that the geometry below is the library's and that the bounds bite -- and tests/test_pointwise_train_gpu.py.

Two kinds of case for every entry point:
  exact    operands are small integers / dyadic numbers (x, dy, W integers, mean integer, invstd, gamma, m1 powers of two, beta,
           m0 dyadic), so every operand, every product and every partial sum in ANY order is an fp32 number: the kernel must
           return the float64 result bit for bit.  exact_margin() is the precondition (sum |terms| < 2^24 quanta per output).
  bounded  random operands, dy spread over four decades (as bn_act_cases.bwd_case): |got - want64| <= bound elementwise.
What cannot be exact: the (mean, M2) tiles of the STATS epilogue (a sum of squared deviations of integers from a mean that is a
multiple of 2^-7 needs more than 24 bits here): y of an exact STATS case is compared bit for bit, its tiles with the bound.
coef = sum / n of mgar_pointwise_conv_dw_bnbwd is a division in double rounded once: the reference does the same operation.

Bounds.  An operand that went through a prologue of r roundings is within gamma_u(r) * A of its float64
value, A = the sum of the magnitudes the prologue adds up (|x - mean| |sc| + |pre| for the BatchNorm prologue, r = 4, as
torch_refs.bn_apply_ref; |k| (|d| + |m0| + |xhat m1|) for the max-pool gradient, r = 7, as torch_refs.bn_bwd_bounds).  The
products run on the exact-fp32 MFMA = an fma chain, so for ANY summation order
    |err| <= gamma_u(d + r) * S + 2^-149,   S = sum |A_a A_b| of the output's terms,
d = the longest chain of additions a term passes through, from the geometry below, never more than the number of terms
(additions of an exact zero do not round).  All numpy; nothing here touches a device."""
import functools

import numpy as np

import bn_act_cases as BC
import torch_refs as R

U32, TINY32, gamma_u = R.U32, R.TINY32, R.gamma_u
F32, F64 = np.float32, np.float64


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ launch geometry, restated
TILE = 128          # DW_TP, PF_COLS: columns per tile
SLICES = 16         # DWR_SLICES, RDR_SLICES of the partial reduces


def dw_blocks(Cin, Cout):
    """dw_blocks() of pointwise_dw.hip: (OB, IB) 32 x 32 output blocks per workgroup."""
    return (1 if Cout <= 32 else 2), (1 if Cin <= 32 else (2 if Cin <= 64 else 4))


def dw_geometry(B, Cin, Cout, P, pair=False, grad=False):
    """Launch of pointwise_dw_kernel<OB, IB, GRAD> for these sizes (pair: the kernel runs on 2 * Cin virtual channels)."""
    cv = 2 * Cin if pair else Cin
    ob, ib = dw_blocks(cv, Cout)
    tiles = B * ceil_div(P, TILE)
    gy, gz = ceil_div(Cout, ob * 32), ceil_div(cv, ib * 32)
    gx = max(min(2048 // (gy * gz), (tiles + 3) // 4), 1)
    n_out = Cout * cv
    # a wave sums 32 columns of each of its workgroup's tiles, wave 0 adds the other three, a reduce slice adds its share of
    # the gx partials, the 16 slices are added in order
    depth = ceil_div(tiles, gx) * 32 + 3 + ceil_div(gx, SLICES) + SLICES
    return dict(ob=ob, ib=ib, grad=grad, pair=pair, tiles=tiles, gx=gx, gy=gy, gz=gz, vec=P % 4 == 0, n_out=n_out,
                workspace=gx * n_out + (n_out if pair else 0), depth=min(depth, max(B * P, 1)),
                instance="dw<%d,%d%s>" % (ob, ib, ",GRAD" if grad else ""),
                staging=("pair_" if pair else "") + ("vector" if P % 4 == 0 else "scalar"))


def rd_geometry(N, Co, Ci):
    """Launch of rowmajor_dw_kernel<OB, IB>: rd_workgroups() sizes the grid by 16-row slabs whatever the instance's own slab."""
    ob, ib = ceil_div(Co, 32), ceil_div(Ci, 32)
    rows = 8 if ob * ib > 6 else 16
    wgs = max(min(ceil_div(ceil_div(N, 16), 32), 256), 1)
    nslab, nwaves = ceil_div(N, rows), 4 * wgs
    depth = ceil_div(nslab, nwaves) * rows + ceil_div(nwaves, SLICES) + SLICES
    return dict(ob=ob, ib=ib, rows=rows, wgs=wgs, nwaves=nwaves, nslab=nslab, idle_waves=max(nwaves - nslab, 0),
                workspace=wgs * 4 * Co * Ci, depth=min(depth, max(N, 1)), instance="rd<%d,%d>" % (ob, ib))


def pf_geometry(B, Cin, Cout, P, stats=False, grad=False):
    """Launch of pointwise_fwd_kernel<OB, float, STATS, GRAD> by launch_pf()."""
    ob = 1 if (Cout <= 32 or stats) else 2
    kc = 16 if ob == 1 else (4 if grad else 8)
    nkc = ceil_div(Cin, kc)
    lds = nkc * kc * ((32 if ob == 1 else 96) + 4 + (1 if grad else 0)) * 4
    ntiles = B * ceil_div(P, TILE)
    wgs = min(ceil_div(ntiles, 4), 2048)
    nwaves = 4 * wgs
    return dict(ob=ob, kc=kc, nkc=nkc, lds=lds, big_lds=lds > 65536, ntiles=ntiles, wgs=wgs, nwaves=nwaves,
                idle_waves=max(nwaves - ntiles, 0), tiles_per_wave=ceil_div(ntiles, nwaves), depth=Cin,
                instance="pf<%d%s%s>" % (ob, ",STATS" if stats else "", ",GRAD" if grad else ""))


# ------------------------------------------------------------------------------------------------ exactness
def quantum(a):
    """The largest power of two that divides every element of a (float64); 1 for an all-zero array."""
    a = np.abs(np.asarray(a, F64)).reshape(-1)
    a = a[a > 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(F64))
    return float(2.0 ** (e - 53 + low).min())


def exact_margin(S, *operands):
    """2^24 * (product of the operands' quanta) / max S: above 1, every partial sum of the output's terms in any order is a
    multiple of the quantum below 2^24 quanta, i.e. an fp32 number."""
    q = 1.0
    for a in operands:
        q *= quantum(a)
    top = float(np.max(S)) if np.size(S) else 0.0
    return np.inf if top == 0 else 2.0 ** 24 * q / top


def roundtrips(a):
    a = np.asarray(a, F64)
    return bool(np.array_equal(a.astype(F32).astype(F64), a))


# ------------------------------------------------------------------------------------------------ operand prologues
ACTS = (None, "both", "none", "gamma_only", "beta_only")     # None: in_mean NULL, the first-layer identity


def _ints(rng, shape, top=4):
    return rng.integers(-top, top + 1, shape).astype(F32)


def _decades(rng, shape):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(F32)


def _pow2(rng, n, exps):
    return (2.0 ** rng.choice(np.asarray(exps, F64), n)).astype(F32)


def exact_bn(rng, C, which, wide=True):
    """BatchNorm vectors whose prologue is exact on integer x: integer mean and beta, invstd and |gamma| powers of two, one
    gamma = 0 (the dead channel) from three channels on.  which: one of ACTS."""
    if which is None:
        return dict(mean=None, invstd=None, gamma=None, beta=None)
    mean = _ints(rng, C, 2)
    invstd = _pow2(rng, C, (-1, 0, 1) if wide else (0, 1))
    gamma = _pow2(rng, C, (-1, 0, 1) if wide else (0, 1)) * rng.choice(np.asarray([-1.0, 1.0], F32), C)
    if C >= 3:
        gamma[2] = 0.0
    beta = _ints(rng, C, 3)
    return dict(mean=mean, invstd=invstd, gamma=gamma if which in ("both", "gamma_only") else None,
                beta=beta if which in ("both", "beta_only") else None)


def random_bn(rng, x, which, relu):
    """mean / invstd = the float64 statistics of x rounded to fp32 (inputs of the entry points), gamma / beta of
    bn_act_cases.affine; under a ReLU x is moved until every pre-activation is RELU_MARGIN off zero (in place)."""
    if which is None:
        return dict(mean=None, invstd=None, gamma=None, beta=None)
    m, v = BC.stats_of(x)
    mean, invstd = m.astype(F32), ((v + BC.EPS) ** -0.5).astype(F32)
    gamma, beta = BC.affine(x.shape[1], which, rng)
    if relu:
        BC.off_threshold(x, mean, invstd, gamma, beta)
    return dict(mean=mean, invstd=invstd, gamma=gamma, beta=beta)


def act_ref(x, k, relu):
    """The X operand: relu?(bn(x)) in float64 of the fp32 vectors of k (mean None: x itself) -> (pre, operand, A, r): A the
    magnitude the prologue's r roundings act on (bn_apply_ref's bound / 4u), A = |x|, r = 0 for the identity."""
    x = np.asarray(x, F64)
    if k["mean"] is None:
        return x, x, np.abs(x), 0
    pre, y, bound = R.bn_apply_ref(x, k["mean"], k["invstd"], k["gamma"], k["beta"], relu)
    return pre, y, bound / (4.0 * U32), 4


def chain_bound(S, d, r):
    return gamma_u(d + r) * np.asarray(S, F64) + TINY32


# ------------------------------------------------------------------------------------------------ forward (and STATS)
FWD_COUT, FWD_CIN = (1, 32, 33, 64), (1, 15, 16, 17, 33, 64, 256)
COLUMNS = ((1, 4), (1, 124), (1, 128), (1, 132), (3, 128), (1, 516), (3, 260))    # (B, P): 1, 1, 1, 2, 3, 5, 9 tiles
BIG_TILES = 8200                                                                   # > 8 192 waves: a wave owns two tiles
BIG_P = TILE * BIG_TILES + 4


def _fwd_table():
    t = {}
    for a, Cout in enumerate(FWD_COUT):
        for b, Cin in enumerate(FWD_CIN):            # exact channel sweep at 6 tiles (two workgroups, two idle waves)
            act = ACTS[(a + b) % len(ACTS)]
            t["x_co%d_ci%d" % (Cout, Cin)] = dict(kind="exact", B=3, Cin=Cin, Cout=Cout, P=132, act=act, relu=(a + b) % 2)
    for B, P in COLUMNS:                             # exact column sweep on <2> with the KC = 8 slab edge
        t["x_cols_b%d_p%d" % (B, P)] = dict(kind="exact", B=B, Cin=17, Cout=33, P=P, act="both", relu=1)
    for Cin, Cout in ((64, 33), (17, 64), (33, 1), (16, 32)):     # W read transposed: the data gradient
        t["x_wt_ci%d_co%d" % (Cin, Cout)] = dict(kind="exact", B=3, Cin=Cin, Cout=Cout, P=132, act=None, relu=0, wt=True)
    t["x_big"] = dict(kind="exact", B=1, Cin=3, Cout=5, P=BIG_P, act=None, relu=0)
    bounded = [(17, 33, 3, 260, "both", 1, False), (64, 64, 1, 516, "none", 1, False), (16, 32, 3, 132, "gamma_only", 0, False),
               (256, 64, 1, 132, "beta_only", 1, False), (33, 1, 1, 4, "both", 1, False), (15, 33, 3, 132, None, 0, True),
               (64, 17, 1, 124, None, 0, True), (1, 64, 1, 128, "both", 0, False), (256, 32, 3, 128, "both", 1, False)]
    for Cin, Cout, B, P, act, relu, wt in bounded:
        t["b_ci%d_co%d_b%d_p%d%s" % (Cin, Cout, B, P, "_wt" if wt else "")] = dict(
            kind="bounded", B=B, Cin=Cin, Cout=Cout, P=P, act=act, relu=relu, wt=wt)
    return t


FWD_CASES = _fwd_table()
STATS_CASES = {
    "x_ci17_co32_b3_p128": dict(kind="exact", B=3, Cin=17, Cout=32, P=128, act="both", relu=1),
    "x_ci33_co1_b1_p640": dict(kind="exact", B=1, Cin=33, Cout=1, P=640, act=None, relu=0),
    "x_big": dict(kind="exact", B=1, Cin=3, Cout=5, P=TILE * BIG_TILES, act=None, relu=0),
    "b_ci17_co32_b3_p128": dict(kind="bounded", B=3, Cin=17, Cout=32, P=128, act="both", relu=1),
    "b_ci15_co5_b1_p640": dict(kind="bounded", B=1, Cin=15, Cout=5, P=640, act="none", relu=1),
}
FWD_REFUSED = {   # (B, Cin, Cout, P): MGAR_EUNSUPPORTED, nothing written
    "p131": (1, 4, 4, 131), "p1": (3, 4, 4, 1), "cout65": (1, 4, 65, 128), "cin257": (1, 257, 4, 128), "cin0": (1, 0, 4, 128),
}


def _seed(family, name):
    return BC._seed(family + ":" + name)


def _conv_case(family, name, spec):
    rng = np.random.default_rng(_seed(family, name))
    B, Cin, Cout, P = spec["B"], spec["Cin"], spec["Cout"], spec["P"]
    exact = spec["kind"] == "exact"
    if exact:
        x, w = _ints(rng, (B, Cin, P)), _ints(rng, (Cout, Cin))
        bn = exact_bn(rng, Cin, spec["act"])
    else:
        x = (0.7 + 2.0 * rng.standard_normal((B, Cin, P), dtype=F32)).astype(F32)
        w = rng.standard_normal((Cout, Cin)).astype(F32)
        bn = random_bn(rng, x, spec["act"], spec["relu"])
    k = dict(spec, name=name, x=x, w=w, wt=spec.get("wt", False), **bn)
    return k, rng


@functools.lru_cache(maxsize=8)
def fwd_case(name):
    k, _ = _conv_case("fwd", name, FWD_CASES[name])
    k["geo"] = pf_geometry(k["B"], k["Cin"], k["Cout"], k["P"])
    return k


@functools.lru_cache(maxsize=8)
def stats_case(name):
    k, _ = _conv_case("stats", name, STATS_CASES[name])
    k["geo"] = pf_geometry(k["B"], k["Cin"], k["Cout"], k["P"], stats=True)
    return k


def w_buffer(k):
    """(the weight as it lies in memory, w_row_stride, w_col_stride) for W[o, i] = buf[o * rs + i * cs]."""
    Cout, Cin = k["w"].shape
    return (np.ascontiguousarray(k["w"].T), 1, Cout) if k.get("wt") else (k["w"], Cin, 1)


def fwd_ref(k, x=None):
    """y = W act(x) in float64 -> dict(y, S, bound, pre, bpre): S = sum_i |W| A_i, bound = chain_bound(S, Cin, r); pre and
    bpre (the prologue's own bound) are what a ReLU case's margin is asserted with."""
    pre, a, A, r = act_ref(k["x"] if x is None else x, k, k["relu"])
    w = k["w"].astype(F64)
    y = np.einsum("oi,bip->bop", w, a)
    S = np.einsum("oi,bip->bop", np.abs(w), A)
    return dict(y=y, S=S, bound=chain_bound(S, k["geo"]["depth"], r), pre=pre, bpre=4.0 * U32 * A + TINY32, operand=a, r=r)


def stats_ref(y32):
    """The (mean, M2) tiles of the fp32 y (B, Cout, P) the kernel wrote, tile = b * (P / 128) + tile of the sample ->
    (tiles (Cout, ntiles, 2) float64, bounds (Cout, ntiles, 2)): torch_refs.qg_tile_stats_ref / qg_tile_stats_bounds, which
    cover the kernel's shape ((v0 + v1) + (v2 + v3), a 5-stage butterfly: 7 roundings for the mean, 10 for M2; they grant
    22 and 25)."""
    y32 = np.asarray(y32, F32)
    B, C, P = y32.shape
    rows = np.ascontiguousarray(y32.transpose(1, 0, 2)).reshape(C, B * P)
    tm, tq, _, _ = R.qg_tile_stats_ref(rows, TILE)
    bm, bq = R.qg_tile_stats_bounds(rows, TILE)
    return np.stack([tm.numpy(), tq.numpy()], 2), np.stack([bm.numpy(), bq.numpy()], 2)


# ------------------------------------------------------------------------------------------------ dW, plain and _act
DW_COUT, DW_CIN = (1, 32, 33, 64, 65, 130), (1, 32, 33, 64, 65, 128, 129)
DW_COLUMNS = ((1, 4), (1, 124), (1, 128), (1, 131), (1, 1), (3, 1), (1, 516), (3, 260), (3, 259), (1, 132))


def _dw_table():
    t = {}
    for a, Cout in enumerate(DW_COUT):
        for b, Cin in enumerate(DW_CIN):             # exact channel sweep, vector and scalar staging alternating
            act = ACTS[(a + 2 * b) % len(ACTS)]
            t["x_co%d_ci%d" % (Cout, Cin)] = dict(kind="exact", B=3, Cin=Cin, Cout=Cout, P=(132, 131)[(a + b) % 2], act=act,
                                                   relu=(a + b + 1) % 2)
    for j, (B, P) in enumerate(DW_COLUMNS):          # exact column sweep on <2,2>: gx = 1, 2, 3
        t["x_cols_b%d_p%d" % (B, P)] = dict(kind="exact", B=B, Cin=33, Cout=33, P=P, act=ACTS[1 + j % 4], relu=j % 2)
    bounded = [(33, 33, 3, 260, "both", 1), (1, 1, 1, 4, "none", 0), (3, 2, 1, 4, "both", 1), (64, 32, 1, 131, "gamma_only", 0),
               (129, 65, 3, 132, "beta_only", 1), (16, 130, 1, 516, None, 0), (65, 1, 3, 1, "both", 0), (17, 33, 3, 259, "both", 1)]
    for Cin, Cout, B, P, act, relu in bounded:
        t["b_ci%d_co%d_b%d_p%d" % (Cin, Cout, B, P)] = dict(kind="bounded", B=B, Cin=Cin, Cout=Cout, P=P, act=act, relu=relu)
    return t


DW_CASES = _dw_table()


@functools.lru_cache(maxsize=8)
def dw_case(name):
    k, rng = _conv_case("dw", name, DW_CASES[name])
    shape = (k["B"], k["Cout"], k["P"])
    k["dy"] = _ints(rng, shape) if k["kind"] == "exact" else _decades(rng, shape)
    k["geo"] = dw_geometry(k["B"], k["Cin"], k["Cout"], k["P"])
    del k["w"]
    return k


def tile_of_columns(B, P):
    """(B, P) int: the tile index b * ceil(P / 128) + p // 128 of every column."""
    return np.arange(B)[:, None] * ceil_div(P, TILE) + np.arange(P)[None, :] // TILE


def dw_ref(k, x=None, dy=None, keep=None):
    """dW[o][i] = sum dy act(x) in float64 -> dict(dw, S, bound).  keep (B, P) 0 / 1 drops columns (the CPU mutants)."""
    pre, a, A, r = act_ref(k["x"] if x is None else x, k, k["relu"])
    dy = np.asarray(k["dy"] if dy is None else dy, F64)
    if keep is not None:
        dy = dy * keep[:, None, :]
    dw = np.einsum("bop,bip->oi", dy, a)
    S = np.einsum("bop,bip->oi", np.abs(dy), A)
    return dict(dw=dw, S=S, bound=chain_bound(S, k["geo"]["depth"], r), pre=pre, bpre=4.0 * U32 * A + TINY32, operand=a, r=r)


def first_slice_columns(geo, B, P):
    """(B, P) 0 / 1: 0 on the columns whose tile goes to a workgroup of reduce slice 0 (tile % gx < ceil(gx / 16))."""
    return (tile_of_columns(B, P) % geo["gx"] >= ceil_div(geo["gx"], SLICES)).astype(F64)


# ------------------------------------------------------------------------------------------------ pair mode: _dw_bnbwd
PAIR_CIN, PAIR_COUT = (1, 16, 17, 32, 33, 64), (1, 33, 64)
PAIR_ACTS = ("both", "none", "gamma_only", "beta_only")


def _pair_table():
    t = {}
    cols = ((3, 132), (3, 131), (3, 260), (1, 4), (1, 1), (1, 516))
    for a, Cout in enumerate(PAIR_COUT):
        for b, Cin in enumerate(PAIR_CIN):
            B, P = cols[(a + b) % len(cols)]
            t["x_ci%d_co%d" % (Cin, Cout)] = dict(kind="exact", B=B, Cin=Cin, Cout=Cout, P=P, act=PAIR_ACTS[(a + b) % 4],
                                                   relu=(a + b + 1) % 2)
    bounded = [(17, 33, 3, 131, "both", 1), (64, 64, 1, 516, "none", 1), (1, 1, 1, 4, "gamma_only", 0),
               (32, 33, 3, 260, "beta_only", 1), (16, 1, 1, 124, "both", 1), (33, 64, 3, 1, "both", 0)]
    for Cin, Cout, B, P, act, relu in bounded:
        t["b_ci%d_co%d_b%d_p%d" % (Cin, Cout, B, P)] = dict(kind="bounded", B=B, Cin=Cin, Cout=Cout, P=P, act=act, relu=relu)
    return t


PAIR_CASES = _pair_table()
PAIR_REFUSED = {"cin65": (1, 65, 4, 128), "cout65": (1, 4, 65, 128)}


@functools.lru_cache(maxsize=8)
def pair_case(name):
    k, rng = _conv_case("pair", name, PAIR_CASES[name])
    shape = (k["B"], k["Cout"], k["P"])
    k["dy"] = _ints(rng, shape) if k["kind"] == "exact" else _decades(rng, shape)
    k["geo"] = dw_geometry(k["B"], k["Cin"], k["Cout"], k["P"], pair=True)
    return k


def pair_ref(k, x=None, force_on=None, keep=None, relu=None):
    """mgar_pointwise_conv_dw_bnbwd in float64: m = [pre > 0] (1 without ReLU; force_on = (b, i, p) sets one element, the
    NaN test's), xhat = (x - mean) invstd, A = sum dy m, B = sum dy m xhat, dW = gamma B + beta A, dbeta_i = sum_o W A,
    dgamma_i = sum_o W B, coef = {dbeta, dgamma} / n.  Bounds: A and B chain_bound with r = 0 and r = 2 (x - mean, * invstd;
    the mask is exact); dW = (1 + g3) (|gamma| bB + |beta| bA) + g3 (|gamma B| + |beta A|), g3 = gamma_u(3): two products and
    an addition; dgamma, dbeta: the sums over o in double on A, B within their bounds, one rounding; coef: the same / n."""
    x = np.asarray(k["x"] if x is None else x, F64)
    relu = k["relu"] if relu is None else relu
    B_, Cin, P = x.shape
    Cout = k["Cout"]
    n = float(B_ * P)
    mu, inv = k["mean"].astype(F64).reshape(1, Cin, 1), k["invstd"].astype(F64).reshape(1, Cin, 1)
    g = np.ones(Cin) if k["gamma"] is None else k["gamma"].astype(F64)
    bt = np.zeros(Cin) if k["beta"] is None else k["beta"].astype(F64)
    xh = (x - mu) * inv
    pre = xh * g.reshape(1, Cin, 1) + bt.reshape(1, Cin, 1)
    m = (pre > 0).astype(F64) if relu else np.ones_like(pre)
    if force_on is not None:
        m[force_on] = 1.0
    dy = k["dy"].astype(F64)
    if keep is not None:
        dy = dy * keep[:, None, :]
    w = k["w"].astype(F64)
    A, Bm = np.einsum("bop,bip->oi", dy, m), np.einsum("bop,bip->oi", dy, m * xh)
    SA, SB = np.einsum("bop,bip->oi", np.abs(dy), m), np.einsum("bop,bip->oi", np.abs(dy), m * np.abs(xh))
    d = k["geo"]["depth"]
    bA, bB = chain_bound(SA, d, 0), chain_bound(SB, d, 2)
    g3 = gamma_u(3)
    ag, ab = np.abs(g)[None, :], np.abs(bt)[None, :]
    dw = g[None, :] * Bm + bt[None, :] * A
    bdw = (1.0 + g3) * (ag * bB + ab * bA) + g3 * (ag * np.abs(Bm) + ab * np.abs(A)) + TINY32
    dbeta, dgamma = (w * A).sum(0), (w * Bm).sum(0)
    bbeta = (np.abs(w) * bA).sum(0) + U32 * np.abs(dbeta) + TINY32
    bgamma = (np.abs(w) * bB).sum(0) + U32 * np.abs(dgamma) + TINY32
    coef = np.stack([dbeta, dgamma], 1) / n
    bcoef = np.stack([(np.abs(w) * bA).sum(0), (np.abs(w) * bB).sum(0)], 1) / n + U32 * np.abs(coef) + TINY32
    return dict(A=A, B=Bm, SA=SA, SB=SB, dw=dw, dgamma=dgamma, dbeta=dbeta, coef=coef, bdw=bdw, bgamma=bgamma, bbeta=bbeta,
                bcoef=bcoef, pre=pre, xh=xh, mask=m, bpre=4.0 * U32 * (np.abs(xh * g.reshape(1, Cin, 1)) + np.abs(pre)) + TINY32)


# ------------------------------------------------------------------------------------------------ GRAD operand mode
# Backward of [conv W (C x Cp) -> BatchNorm -> ReLU -> max over ns]: C = channels of the max-pool layer (x4), Cp = channels of
# the layer in front (x).  mgar_pointwise_conv_fwd_maxgrad: dX (B, Cp, P) = W^T dx4 (Cin = C, Cout = Cp, W read transposed);
# mgar_pointwise_conv_dw_maxgrad: dW (C, Cp) = sum dx4 act(x) (Cin = Cp, Cout = C).
GRAD_CASES = {
    # bounded: coef and dmask come from mgar_bn_act_maxpool_bwd_reduce on the device, the dense dx4 from mgar_bn_act_maxpool_bwd
    "b_ns4_m1": dict(kind="bounded", B=1, C=5, Cp=3, M=1, ns=4, gamma="mixed", act="both", relu=1),
    "b_ns4_m11": dict(kind="bounded", B=3, C=33, Cp=33, M=11, ns=4, gamma="mixed", act="none", relu=1),
    "b_ns12_m1": dict(kind="bounded", B=3, C=7, Cp=40, M=1, ns=12, gamma="mixed", act=None, relu=0),
    "b_ns12_m11": dict(kind="bounded", B=1, C=64, Cp=16, M=11, ns=12, gamma="mixed", act="gamma_only", relu=0),
    "b_ns128_m1": dict(kind="bounded", B=1, C=4, Cp=64, M=1, ns=128, gamma="mixed", act="beta_only", relu=1),
    "b_ns128_m11": dict(kind="bounded", B=3, C=40, Cp=8, M=11, ns=128, gamma=None, act="both", relu=1),
    "b_ns252_m1": dict(kind="bounded", B=3, C=6, Cp=6, M=1, ns=252, gamma="mixed", act="both", relu=0),
    "b_ns252_m11": dict(kind="bounded", B=1, C=36, Cp=64, M=11, ns=252, gamma="mixed", act="both", relu=1),
    "b_big": dict(kind="bounded", B=1, C=3, Cp=5, M=BIG_P // 12, ns=12, gamma="mixed", act=None, relu=0, fwd_only=True),
    # exact: coef, dmask and arg are the test's own
    "x_ns4_m1": dict(kind="exact", B=1, C=5, Cp=3, M=1, ns=4, gamma="mixed", act="both", relu=1),
    "x_ns12_m11": dict(kind="exact", B=3, C=33, Cp=17, M=11, ns=12, gamma="mixed", act="both", relu=1),
    "x_ns128_m11": dict(kind="exact", B=3, C=5, Cp=64, M=11, ns=128, gamma=None, act=None, relu=0),
    "x_ns252_m1": dict(kind="exact", B=3, C=64, Cp=33, M=1, ns=252, gamma="mixed", act="gamma_only", relu=1),
    "x_ns252_m11": dict(kind="exact", B=1, C=17, Cp=64, M=11, ns=252, gamma="mixed", act="beta_only", relu=0),
}
assert BIG_P % 12 == 0
GRAD_REFUSED = {"c65": dict(C=65, Cp=4, ns=4), "cp65": dict(C=4, Cp=65, ns=4), "ns6": dict(C=4, Cp=4, ns=6)}


def planted_slots(M, ns):
    """[(channels, group, slot)] the arg-max is put at: slot 0 in group 0, slot ns - 1 in group 1 and -- where a group
    straddles a 128-column tile -- a slot behind the tile edge, in every channel; with one group, slot 0 in channel 0 and slot
    ns - 1 in channel 1."""
    if M == 1:
        return [(slice(0, 1), 0, 0), (slice(1, 2), 0, ns - 1)]
    plant = [(slice(None), 0, 0), (slice(None), 1, ns - 1)]
    for m in range(2, M):
        lo, hi = m * ns, (m + 1) * ns - 1
        if lo // TILE != hi // TILE:
            plant.append((slice(None), m, ((lo // TILE + 1) * TILE - lo) + min(1, hi % TILE)))   # first or second column behind it
            break
    return plant


def _pool_gamma(rng, C, which, exact):
    """gamma of the max-pool layer's BatchNorm: positive, negative, exactly 0, positive (a channel whose beta keeps it dead
    under the ReLU), cycling; None = NULL."""
    mag = _pow2(rng, C, (0, 1)) if exact else rng.uniform(0.5, 1.5, C).astype(F32)
    sign = np.array([1.0, -1.0, 0.0, 1.0], F32)[np.arange(C) % 4]
    beta = np.array([0.25, -0.25, 0.5, -40.0], F32)[np.arange(C) % 4]
    return (None if which is None else mag * sign), beta


@functools.lru_cache(maxsize=4)
def grad_case(name):
    """x4 (B, C, M, ns), x (B, Cp, P), w (C, Cp), the pool layer's mean / invstd / gamma / beta and the X operand's BatchNorm.
    bounded: the forward state (pooled, arg, xarg) of float64 BatchNorm -> ReLU -> max with the arg-max planted as
    planted_slots() says, dpool over four decades; channel 3 (mod 4) has beta = -40: pooled = 0, dmask zero everywhere.
    exact: coef, dmask, arg are inputs, all dyadic."""
    spec = GRAD_CASES[name]
    rng = np.random.default_rng(_seed("grad", name))
    B, C, Cp, M, ns = spec["B"], spec["C"], spec["Cp"], spec["M"], spec["ns"]
    P = M * ns
    exact = spec["kind"] == "exact"
    k = dict(spec, name=name, P=P)
    gamma, beta = _pool_gamma(rng, C, spec["gamma"], exact)
    plant = planted_slots(M, ns)
    if exact:
        x4, x, w = _ints(rng, (B, C, M, ns), 2), _ints(rng, (B, Cp, P), 2), _ints(rng, (C, Cp))
        mean, invstd = _ints(rng, C, 2), _pow2(rng, C, (0, 1))
        coef = np.stack([_ints(rng, C, 2) * F32(0.5), _pow2(rng, C, (-1, 0)) * rng.choice(np.asarray([-1.0, 1.0], F32), C)], 1)
        arg = rng.integers(0, ns, (B, C, M)).astype(np.uint8)
        for cs, m, s in plant:
            arg[:, cs, m] = s
        dmask = _ints(rng, (B, C, M))
        dmask[:, 3::4] = 0.0
        k.update(coef=coef.astype(F32), arg=arg, dmask=dmask, **{"in_" + a: v for a, v in exact_bn(rng, Cp, spec["act"], wide=False).items()})
    else:
        x4 = (0.7 + 2.0 * rng.standard_normal((B, C, M, ns), dtype=F32)).astype(F32)
        x = (0.7 + 2.0 * rng.standard_normal((B, Cp, P), dtype=F32)).astype(F32)
        w = rng.standard_normal((C, Cp)).astype(F32)
        m_, v_ = BC.stats_of(x4.reshape(B, C, P))
        mean, invstd = m_.astype(F32), ((v_ + BC.EPS) ** -0.5).astype(F32)
        g = np.ones(C, F32) if gamma is None else gamma
        for cs, m, s in plant:           # the extreme of the group, moved out by 1, copied into the slot
            up = (g >= 0)[None, cs]
            x4[:, cs, m, s] = np.where(up, x4[:, cs, m].max(-1) + 1.0, x4[:, cs, m].min(-1) - 1.0)
        BC.off_threshold(x4.reshape(B, C, P), mean, invstd, gamma, beta)
        pre, _, bound = R.bn_apply_ref(x4.reshape(B, C, P), mean, invstd, gamma, beta, 0)
        pre = pre.reshape(B, C, M, ns)
        pooled, arg = R.bn_max_ref(pre, 1)
        for cs, m, s in plant:
            live = np.arange(C)[cs][g[cs] != 0]
            assert (arg[:, live, m] == s).all(), (name, m, s)
        arg8 = arg.astype(np.uint8)
        k.update(pooled=pooled.astype(F32), arg=arg8, xarg=np.take_along_axis(x4, arg[..., None], -1)[..., 0],
                 dpool=_decades(rng, (B, C, M)), pre4=pre, bpre4=bound.reshape(B, C, M, ns),
                 **{"in_" + a: v for a, v in random_bn(rng, x, spec["act"], spec["relu"]).items()})
    k.update(x4=x4, x=x, w=w, mean=mean, invstd=invstd, gamma=gamma, beta=beta, plant=plant,
             geo_fwd=pf_geometry(B, C, Cp, P, grad=True), geo_dw=dw_geometry(B, Cp, C, P, grad=True))
    return k


def dx4_ref(k, coef, dmask, arg=None, x4=None, swap=False):
    """The max-pool layer's input gradient in float64 of its fp32 inputs, coef / dmask / arg included:
    dx4 = k (onehot(arg) d - m0 - xhat m1), k = gamma invstd -> (dx4 (B, C, P), A): A = |k| (|d at arg| + |m0| + |xhat m1|),
    what its 7 roundings act on (torch_refs.bn_bwd_bounds, coef given).  swap exchanges m0 and m1 (a CPU mutant)."""
    x4 = np.asarray(k["x4"] if x4 is None else x4, F64)
    arg = np.asarray(k["arg"] if arg is None else arg).astype(np.int64)
    B, C, M, ns = x4.shape
    coef = np.asarray(coef, F64).reshape(C, 2)
    m0, m1 = (coef[:, 1], coef[:, 0]) if swap else (coef[:, 0], coef[:, 1])
    mu, inv = k["mean"].astype(F64).reshape(1, C, 1, 1), k["invstd"].astype(F64).reshape(1, C, 1, 1)
    g = np.ones(C) if k["gamma"] is None else k["gamma"].astype(F64)
    kk = inv * g.reshape(1, C, 1, 1)
    d = np.zeros(x4.shape)
    np.put_along_axis(d, arg[..., None], np.asarray(dmask, F64).reshape(B, C, M, 1), -1)
    xh = (x4 - mu) * inv
    t0, t1 = m0.reshape(1, C, 1, 1), xh * m1.reshape(1, C, 1, 1)
    dx = kk * (d - t0 - t1)
    A = np.abs(kk) * (np.abs(d) + np.abs(t0) + np.abs(t1))
    return dx.reshape(B, C, M * ns), A.reshape(B, C, M * ns)


def fwd_maxgrad_ref(k, coef, dmask, **kw):
    """dX[b, j, p] = sum_c W[c, j] dx4[b, c, p] -> dict(y, S, bound), r = 7."""
    dx, A = dx4_ref(k, coef, dmask, **kw)
    w = k["w"].astype(F64)
    S = np.einsum("cj,bcp->bjp", np.abs(w), A)
    return dict(y=np.einsum("cj,bcp->bjp", w, dx), S=S, bound=chain_bound(S, k["geo_fwd"]["depth"], 7), operand=dx)


def grad_act(k, x=None):
    return act_ref(k["x"] if x is None else x, dict(mean=k["in_mean"], invstd=k["in_invstd"], gamma=k["in_gamma"],
                                                    beta=k["in_beta"]), k["relu"])


def dw_maxgrad_ref(k, coef, dmask, x=None, keep=None, **kw):
    """dW[c, j] = sum dx4[b, c, p] act(x)[b, j, p] -> dict(dw, S, bound), r = 7 + (4 or 0)."""
    dx, A = dx4_ref(k, coef, dmask, **kw)
    pre, a, Ax, r = grad_act(k, x)
    if keep is not None:
        dx, A = dx * keep[:, None, :], A * keep[:, None, :]
    S = np.einsum("bcp,bjp->cj", A, Ax)
    return dict(dw=np.einsum("bcp,bjp->cj", dx, a), S=S, bound=chain_bound(S, k["geo_dw"]["depth"], 7 + r), pre=pre,
                bpre=4.0 * U32 * Ax + TINY32, operand=a, r=r)


# ------------------------------------------------------------------------------------------------ rowmajor_dw
RD_CO, RD_CI, RD_N = (1, 33, 96), (5, 33, 65, 128), (1, 15, 16, 17, 300)


def _rd_table():
    t = {}
    for a, Co in enumerate(RD_CO):
        for b, Ci in enumerate(RD_CI):
            for j in (0, 2):                          # every instance at two N, padded and tight leading dimensions
                N = RD_N[(a * len(RD_CI) + b + j) % len(RD_N)]
                t["x_co%d_ci%d_n%d" % (Co, Ci, N)] = dict(kind="exact", Co=Co, Ci=Ci, N=N, pad=(a + b + j // 2) % 2)
    for Co, Ci, N, pad in ((33, 65, 300, 1), (96, 128, 300, 0), (1, 5, 17, 1), (96, 33, 15, 1)):
        t["b_co%d_ci%d_n%d" % (Co, Ci, N)] = dict(kind="bounded", Co=Co, Ci=Ci, N=N, pad=pad)
    return t


RD_CASES = _rd_table()
RD_REFUSED = {"co97": (97, 4, -3), "ci129": (4, 129, -3)}     # (Co, Ci, code); lda < Co is MGAR_EINVAL


@functools.lru_cache(maxsize=8)
def rd_case(name):
    """a (N, lda), f (N, ldf) with lda = Co + 5, ldf = Ci + 3 when padded; the padding columns hold 1e30 (exact cases: 2^20),
    which no instance may read into a sum."""
    spec = RD_CASES[name]
    rng = np.random.default_rng(_seed("rd", name))
    Co, Ci, N = spec["Co"], spec["Ci"], spec["N"]
    lda, ldf = (Co + 5, Ci + 3) if spec["pad"] else (Co, Ci)
    exact = spec["kind"] == "exact"
    a = np.full((N, lda), 2.0 ** 20 if exact else 1e30, F32)
    f = np.full((N, ldf), 2.0 ** 20 if exact else 1e30, F32)
    a[:, :Co] = _ints(rng, (N, Co)) if exact else _decades(rng, (N, Co))
    f[:, :Ci] = _ints(rng, (N, Ci)) if exact else rng.standard_normal((N, Ci)).astype(F32)
    return dict(spec, name=name, a=a, f=f, lda=lda, ldf=ldf, geo=rd_geometry(N, Co, Ci))


def rd_ref(k, keep=None):
    a, f = k["a"][:, :k["Co"]].astype(F64), k["f"][:, :k["Ci"]].astype(F64)
    if keep is not None:
        a = a * keep[:, None]
    S = np.abs(a).T @ np.abs(f)
    return dict(dw=a.T @ f, S=S, bound=chain_bound(S, k["geo"]["depth"], 0))


# ------------------------------------------------------------------------------------------------ what the cases reach
def reach_table():
    """{what: [case ids]} for every instance and path the issue lists, read off the restated geometry of every case."""
    t = {}

    def add(what, case):
        t.setdefault(what, []).append(case)

    for n, s in FWD_CASES.items():
        g = pf_geometry(s["B"], s["Cin"], s["Cout"], s["P"])
        add(g["instance"] + " plain", "fwd:" + n)
        add("pf slab KC=%d nkc=%d" % (g["kc"], g["nkc"]), "fwd:" + n)
        if g["big_lds"]:
            add("pf LDS above 64 KB", "fwd:" + n)
        if g["tiles_per_wave"] > 1:
            add("pf more than one tile per wave, plain", "fwd:" + n)
        if g["idle_waves"]:
            add("pf idle waves", "fwd:" + n)
        if g["ntiles"] < 4:
            add("pf ntiles < 4", "fwd:" + n)
        if s["P"] < TILE:
            add("pf P < 128", "fwd:" + n)
        if s["P"] % TILE:
            add("pf tail tile", "fwd:" + n)
        if s.get("wt"):
            add("pf W transposed", "fwd:" + n)
    for n, s in STATS_CASES.items():
        g = pf_geometry(s["B"], s["Cin"], s["Cout"], s["P"], stats=True)
        add(g["instance"], "stats:" + n)
        if g["tiles_per_wave"] > 1:
            add("pf more than one tile per wave, STATS", "stats:" + n)
    for n, s in DW_CASES.items():
        g = dw_geometry(s["B"], s["Cin"], s["Cout"], s["P"])
        add(g["instance"], "dw:" + n)
        add("dw staging " + g["staging"], "dw:" + n)
        add("dw gx=%d" % g["gx"], "dw:" + n)
        if g["gy"] > 1:
            add("dw gy > 1", "dw:" + n)
        if g["gz"] > 1:
            add("dw gz > 1", "dw:" + n)
        if s["act"] is not None and not s["relu"]:
            add("dw_act in_relu = 0", "dw:" + n)
        if s["act"] in ("none", "gamma_only", "beta_only"):
            add("dw_act gamma / beta NULL", "dw:" + n)
        if s["P"] < TILE:
            add("dw P < 128", "dw:" + n)
    for n, s in PAIR_CASES.items():
        g = dw_geometry(s["B"], s["Cin"], s["Cout"], s["P"], pair=True)
        add(g["instance"] + " pair", "pair:" + n)
        add("dw staging " + g["staging"], "pair:" + n)
    for n, s in GRAD_CASES.items():
        P = s["M"] * s["ns"]
        g = pf_geometry(s["B"], s["C"], s["Cp"], P, grad=True)
        add(g["instance"], "grad:" + n)
        if g["tiles_per_wave"] > 1:
            add("pf more than one tile per wave, GRAD", "grad:" + n)
        if not s.get("fwd_only"):
            add(dw_geometry(s["B"], s["Cp"], s["C"], P, grad=True)["instance"], "grad:" + n)
        if s["ns"] > 128:
            add("GRAD arg bytes above 127", "grad:" + n)
        if any(m >= 2 for _, m, _ in planted_slots(s["M"], s["ns"])):
            add("GRAD group straddles a tile, arg behind the edge", "grad:" + n)
        if s["gamma"] is None:
            add("GRAD gamma NULL", "grad:" + n)
    for n, s in RD_CASES.items():
        g = rd_geometry(s["N"], s["Co"], s["Ci"])
        add(g["instance"], "rd:" + n)
        if g["idle_waves"] >= 3:
            add("rd three idle waves", "rd:" + n)
        if s["pad"]:
            add("rd padded leading dimensions", "rd:" + n)
    return t


REACH_REQUIRED = (
    ["dw<%d,%d>" % (o, i) for o in (1, 2) for i in (1, 2, 4)] + ["dw<%d,%d> pair" % (o, i) for o in (1, 2) for i in (1, 2, 4)]
    + ["dw<%d,%d,GRAD>" % (o, i) for o in (1, 2) for i in (1, 2)] + ["rd<%d,%d>" % (o, i) for o in (1, 2, 3) for i in (1, 2, 3, 4)]
    + ["pf<1> plain", "pf<2> plain", "pf<1,STATS>", "pf<1,GRAD>", "pf<2,GRAD>", "pf LDS above 64 KB",
       "pf more than one tile per wave, plain", "pf more than one tile per wave, STATS", "pf more than one tile per wave, GRAD",
       "pf idle waves", "pf ntiles < 4", "pf P < 128", "pf tail tile", "pf W transposed",
       "pf slab KC=16 nkc=1", "pf slab KC=16 nkc=2", "pf slab KC=16 nkc=16", "pf slab KC=8 nkc=1", "pf slab KC=8 nkc=2",
       "pf slab KC=8 nkc=3", "pf slab KC=8 nkc=32",
       "dw staging vector", "dw staging scalar", "dw staging pair_vector", "dw staging pair_scalar", "dw gx=1", "dw gx=2", "dw gx=3",
       "dw gy > 1", "dw gz > 1", "dw_act in_relu = 0", "dw_act gamma / beta NULL", "dw P < 128",
       "GRAD arg bytes above 127", "GRAD group straddles a tile, arg behind the edge", "GRAD gamma NULL",
       "rd three idle waves", "rd padded leading dimensions"])
