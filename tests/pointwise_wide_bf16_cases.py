"""Cases, operands, float64 reference and per-element bounds shared by tests/test_pointwise_wide_bf16_cpu.py and
tests/test_pointwise_wide_bf16_gpu.py for mgar_pointwise_wide_bf16_fwd / mgar_pointwise_wide_maxpool_bf16_fwd
(csrc/pointwise_wide_bf16.hip).

The kernel's contract (include/mgar_ops.h):
    a[b,i,p] = bf16(act_i(float(x[b,i,p])))   act_i(v) = relu?(((v - mean_i) * sc_i) + beta_i), sc_i = invstd_i * gamma_i, every
                                              operation rounded to fp32 on its own; identity prologue: a = x
    w~[o,i]  = bf16(w[o * w_ld + i])
    acc      = sum_i w~[o,i] * a[b,i,p]       fp32 accumulation of exact products
    plain :  y[b,o,p] = bf16(acc)
    affine:  y[b,o,p] = bf16(relu?(fmaf(acc, scale_o, shift_o)))
    pooled:  y[b,o,m] = bf16(max_{s<ns} relu?(fmaf(acc[b,o,m*ns+s], scale_o, shift_o)))
The rounded operands are restated in torch as tests/pointwise_bf16_cases.py does (its `activated`); the reference is the float64
chain on them.  No new tolerance:
    plain   pointwise_bf16_cases.reference:  B + 2^-8 (|ref| + B),  B = gamma(2 (Cin + 2)) S,  S = sum_i |w~| |a|
    affine  sparse_conv_affine_cases.bound(z, S, Cin, scale, shift, relu, bf16=True) = E + 2^-8 (|ref| + E),
            E = |scale| B + 2 u (|z scale| + |shift|) + 1e-30, as tests/conv1x1_bf16_cases.py uses it
    pooled  E_out = max over the group of that E (max is 1-Lipschitz, as tests/mlp_eval_cases.py), then the one rounding:
            E_out + 2^-8 (|ref| + E_out)
Everything here runs on the CPU and is computed once per (case, variant)."""
import functools

import numpy as np
import torch

import pointwise_bf16_cases as PC
import sparse_conv_affine_cases as A

BF = torch.bfloat16
BF16_EPS = 2.0 ** -8

# (B, Cin, Cout, P, weight slice): None = W is a contiguous (Cout, Cin) matrix; (ld, c0) = W is the column slice [:, c0 : c0 + Cin]
# of a (Cout, ld) matrix -- w_ld = ld and the pointer is c0 floats behind a 16-byte boundary
CASES = (
    (1, 1, 1, 4, None),            # the minimum
    (2, 17, 65, 132, None),        # ragged k-step; a third row block holding one row; ragged second tile
    (1, 99, 64, 256, None),        # Cin odd: W is loaded without vectors; wide only by Cin
    (2, 128, 33, 516, None),       # wide only by Cin; half-empty second row block
    (1, 259, 128, 128, None),      # odd Cin; W in more than one LDS chunk
    (3, 196, 256, 644, None),      # tiles straddle samples
    (2, 1024, 512, 260, None),     # both limits, the largest instance, many chunks
    (1, 384, 512, 8, None),        # fewer tiles than a workgroup's tile slots
    (2, 61, 96, 512, (160, 3)),    # the weight slice [:, 3:64] of a (96, 160) matrix
)
PROLOGUES = PC.VARIANTS            # "identity", "bn_relu", "bn_noaffine"
STORES = ("plain", "affine_relu", "affine")

# (B, Cin, Cout, M, ns), prologue, out_relu: the switches rotated
POOLED = (
    ((1, 64, 128, 8, 4), "bn_relu", 1),
    ((2, 196, 256, 33, 16), "identity", 1),
    ((3, 128, 65, 100, 32), "bn_noaffine", 0),
    ((2, 17, 96, 7, 64), "bn_relu", 0),
    ((1, 256, 512, 5, 128), "bn_noaffine", 1),
)


def case_id(case):
    b, cin, cout, p, sl = case
    return "%dx%dx%dx%d%s" % (b, cin, cout, p, "" if sl is None else "_ld%d_c%d" % sl)


def pooled_id(pc):
    (b, cin, cout, m, ns), pro, orl = pc
    return "%dx%dx%dx%dx%d_%s_r%d" % (b, cin, cout, m, ns, pro, orl)


def pooled_as_case(pc):
    """the unpooled case that holds a pooled case's operands: P = M * ns"""
    (b, cin, cout, m, ns), _, _ = pc
    return (b, cin, cout, m * ns, None)


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def operands(case, prologue):
    """-> dict of CPU tensors: x (B, Cin, P) bf16; w_full (Cout, ld) fp32 as stored, w_ld, w_off (floats from w_full's start to
    W[0, 0]), w (Cout, Cin) fp32 logical; mean, invstd, gamma | None, beta | None (Cin) fp32; relu.  The recipe of
    pointwise_bf16_cases.operands: randn x, W scaled by 0.2, invstd >= 0.5."""
    b, cin, cout, p, sl = case
    seed = 10 * (b + 131 * cin + 1009 * cout + 7 * p) + 100003 * PROLOGUES.index(prologue)
    ld, c0 = sl if sl is not None else (cin, 0)
    x = _rnd(b, cin, p, seed=seed + 1).to(BF)
    w_full = _rnd(cout, ld, seed=seed + 2, scale=0.2).contiguous()
    ops = {"x": x, "w_full": w_full, "w_ld": ld, "w_off": c0, "w": w_full[:, c0:c0 + cin].contiguous(), "relu": 0, "mean": None,
           "invstd": None, "gamma": None, "beta": None}
    if prologue != "identity":
        ops["mean"] = _rnd(cin, seed=seed + 3, scale=0.1)
        ops["invstd"] = _rnd(cin, seed=seed + 4).abs() + 0.5
    if prologue == "bn_relu":
        ops["gamma"] = _rnd(cin, seed=seed + 5) * 0.1 + 1
        ops["beta"] = _rnd(cin, seed=seed + 6) * 0.1
        ops["relu"] = 1
    return ops


def rounded_operands(ops):
    """-> (a (B, Cin, P), w~ (Cout, Cin)) as fp32 tensors holding bf16 values"""
    return PC.rounded_operands(ops)


def per_channel(v):
    return np.asarray(v).reshape(1, -1, 1)


def affine_params(seed, z):
    """scale, shift (Cout) float32 for the float64 product z (B, Cout, P): the recipe of i3d_fold_bn_cases.affine_params for any
    channel count -- scale of mixed sign over 10^U(-2, 2) with a negative entry at channel 0, an exact zero at channel 1 (and every
    fifth from there) and a large one (1000) at channel 2, where those channels exist; shift = half the channel's median |z scale|
    times a standard normal (a standard normal where that is 0): roughly half of the pre-activations are negative."""
    rng = np.random.default_rng(seed)
    c = z.shape[1]
    scale = (rng.choice([-1.0, 1.0], c) * 10.0 ** rng.uniform(-2, 2, c)).astype(np.float32)
    scale[0] = -abs(scale[0])
    scale[1::5] = 0.0
    if c > 2:
        scale[2] = 1000.0
    zc = np.moveaxis(z, 1, 0).reshape(c, -1)
    spread = np.median(np.abs(zc * scale.astype(np.float64)[:, None]), axis=1)
    shift = (np.where(spread > 0, 0.5 * spread, 1.0) * rng.standard_normal(c)).astype(np.float32)
    return scale, shift


def pooled_shift(z, scale, ns, seed):
    """shift (Cout) float32 for the pooled store, the recipe of mlp_eval_cases.make_case: even channels minus a cut between two
    adjacent group maxima of z scale, the one that leaves about 30 % -- at least one -- of the channel's groups with every value
    below 0, so that out_relu zeroes whole groups; odd channels plus 0.2 .. 0.4 of the channel's standard deviation."""
    rng = np.random.default_rng(seed)
    b, cout, p = z.shape
    zs = (z * scale.astype(np.float64)[None, :, None]).reshape(b, cout, p // ns, ns)
    gmax = np.sort(zs.max(axis=3).transpose(1, 0, 2).reshape(cout, -1), axis=1)
    k = min(max(1, int(round(0.3 * gmax.shape[1]))), gmax.shape[1] - 1)
    spread = zs.std(axis=(0, 2, 3)) * rng.uniform(0.2, 0.4, cout)
    shift = -0.5 * (gmax[:, k - 1] + gmax[:, k])
    shift = np.where(gmax[:, k - 1] == gmax[:, k], -(gmax[:, k] + spread), shift)
    shift[1::2] = spread[1::2]
    return shift.astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(case, prologue):
    """-> dict: ref, bound (float64 tensors, the plain store); z, S (float64 numpy (B, Cout, P)); scale, shift (float32 numpy
    (Cout), the affine stores).  Computed once and shared: callers must not modify it."""
    a, wt = rounded_operands(operands(case, prologue))
    ref, bound = PC.reference(a, wt)
    z = ref.numpy()
    S = torch.einsum("oi,bip->bop", wt.double().abs(), a.double().abs()).numpy()
    scale, shift = affine_params(sum(case[:4]) + PROLOGUES.index(prologue), z)
    for v in (z, S, scale, shift):
        v.setflags(write=False)
    return dict(ref=ref, bound=bound, z=z, S=S, scale=scale, shift=shift)


@functools.lru_cache(maxsize=None)
def affine_expected(case, prologue, relu):
    """-> (float64 reference, bound) of the affine store, numpy (B, Cout, P), read-only"""
    e = expected(case, prologue)
    sc, sh = per_channel(e["scale"]), per_channel(e["shift"])
    ref, bound = A.reference(e["z"], sc, sh, relu), A.bound(e["z"], e["S"], case[1], sc, sh, relu, True)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def store_expected(case, prologue, store):
    """-> (ref, bound) as float64 numpy for any of STORES"""
    if store == "plain":
        e = expected(case, prologue)
        return e["ref"].numpy(), e["bound"].numpy()
    return affine_expected(case, prologue, store == "affine_relu")


def store_args(case, prologue, store):
    """-> (scale | None, shift | None, out_relu) of a store variant, float32 numpy"""
    if store == "plain":
        return None, None, 0
    e = expected(case, prologue)
    return e["scale"], e["shift"], int(store == "affine_relu")


@functools.lru_cache(maxsize=None)
def pooled_expected(pc):
    """-> dict: ref, bound (float64 numpy (B, Cout, M)); v, E (float64 numpy (B, Cout, M, ns): the affine values and their bound
    before the store rounding); scale, shift (float32 numpy (Cout)).  Read-only."""
    (b, cin, cout, m, ns), prologue, orl = pc
    case = pooled_as_case(pc)
    e = expected(case, prologue)
    scale = e["scale"]
    shift = pooled_shift(e["z"], scale, ns, 5 + sum(pc[0]))
    sc, sh = per_channel(scale), per_channel(shift)
    v = A.reference(e["z"], sc, sh, orl)
    # the affine bound before the store rounding: A.bound(.., bf16=True) = E + 2^-8 (|v| + E), solved for E
    E = (A.bound(e["z"], e["S"], cin, sc, sh, orl, True) - BF16_EPS * np.abs(v)) / (1.0 + BF16_EPS)
    v, E = v.reshape(b, cout, m, ns), E.reshape(b, cout, m, ns)
    ref, e_out = v.max(axis=3), E.max(axis=3)
    bound = e_out + BF16_EPS * (np.abs(ref) + e_out)
    for t in (ref, bound, v, E, shift):
        t.setflags(write=False)
    return dict(ref=ref, bound=bound, v=v, E=E, scale=scale, shift=shift)


def share(y, ref, bound):
    """largest |y - ref| / bound over the elements (float64 numpy); an element whose bound is 0 must be exact"""
    err = np.abs(np.asarray(y, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0
