"""Value cases, bounds and numpy emulation of the op-level tests of the affine [+ ReLU] store of csrc/sparse_conv.hip and
csrc/sparse_conv_bf16.hip (mgar_spconv_gather_gemm_affine / mgar_spconv_bf16_fwd_affine), shared by
tests/test_sparse_conv_affine_cpu.py (the bounds are satisfiable: no kernel involved) and tests/test_sparse_conv_affine_gpu.py.
Tables, seeds and the float64 gather-GEMM come from tests/sparse_conv_cases.py and tests/sparse_conv_bf16_cases.py unchanged.

Contract under test, with acc the fp32 accumulator of the plain entry point: v = fmaf(acc, scale[c], shift[c]);
out = relu ? max(v, +0) with a NaN passed through : v; the bf16 entry rounds out once.  Reference, in float64: z = gather_gemm_ref
(on the rounded operands for bf16), ref = act(z * scale + shift).  Per element, with B the accumulation bound of the respective
plain kernel (cases.bound(n, 2, S) for fp32; gamma(2 (n + 2)) S for bf16) and u = 2^-24:
    fp32:  |got - ref| <= E = |scale| B + 2 u (|z scale| + |shift|) + 1e-30
    bf16:  |got - ref| <= E + 2^-8 (|ref| + E)
|scale| B is the accumulator's error carried through the multiplication, 2 u (|z scale| + |shift|) covers the one rounding of the
fma (u |v| <= u (|z scale| + |shift|) (1 + ...)) with a factor 2 of slack, 2^-8 is the one rounding to bf16 of a value within E of
ref.  The ReLU is 1-Lipschitz, so the same bound holds behind it."""
import functools

import numpy as np

import sparse_conv_bf16_cases as B
import sparse_conv_cases as C

U = 2.0 ** -24


def fp32_plan_cases():
    """name -> (table, C_in, C_out, flip_k, seed): every channel plan of sparse_conv_cases.PLANS (register float4, register
    scalar, LDS, big-LDS 128 x 128) on the 193-row submanifold table."""
    return {"fp32plan_%dx%d" % (cin, cout): (B.subm_table(C.PLAN_ROWS), cin, cout, 0, 7000 + 131 * cin + cout) for cin, cout in C.PLANS}


def value_cases(bf16):
    """The cases of sparse_conv_bf16_cases.value_cases(); for fp32 also fp32_plan_cases()."""
    out = dict(B.value_cases())
    if not bf16:
        out.update(fp32_plan_cases())
    return out


def affine_params(rng, z):
    """scale, shift (C_out) float32 for a float64 product z (No, C_out): scale of mixed sign over 10^U(-2, 2) with every fifth
    channel (from channel 1) exactly 0; shift = half the channel's median |z scale| times a standard normal (a standard normal
    where that is 0), so that roughly half of the pre-activations z scale + shift are negative."""
    cout = z.shape[1]
    scale = (rng.choice([-1.0, 1.0], cout) * 10.0 ** rng.uniform(-2, 2, cout)).astype(np.float32)
    scale[1::5] = 0.0
    spread = np.median(np.abs(z * scale.astype(np.float64)), axis=0) if z.shape[0] else np.zeros(cout)
    shift = (np.where(spread > 0, 0.5 * spread, 1.0) * rng.standard_normal(cout)).astype(np.float32)
    return scale, shift


@functools.lru_cache(maxsize=None)
def case(name, bf16):
    """-> dict(nbr, x, w, flip, scale, shift, z, S, n): operands (bf16-valued float32 for bf16), the float64 product and its
    |.|-sum and term count.  Computed once per case and shared: treat as read-only."""
    nbr, cin, cout, flip, seed = value_cases(bf16)[name]
    rng = np.random.default_rng(seed)
    n_src = int(nbr.max()) + 1 if nbr.size and nbr.max() >= 0 else 1
    x = C.wide_range(rng, (max(n_src, nbr.shape[0]), cin))
    w = C.weights(rng, nbr.shape[1], cin, cout)
    if bf16:
        x, w = B.to_bf16(x), B.to_bf16(w)
    z, S, n = C.gather_gemm_ref(nbr, x, w, flip)
    scale, shift = affine_params(np.random.default_rng(seed + 1), z)
    out = dict(nbr=nbr, x=x, w=w, flip=flip, scale=scale, shift=shift, z=z, S=S, n=n)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def act(v, relu):
    """float64 ReLU that passes a NaN (np.maximum does) -- or the identity"""
    return np.maximum(v, 0.0) if relu else v


def reference(z, scale, shift, relu):
    return act(z * scale.astype(np.float64) + shift.astype(np.float64), relu)


def bound(z, S, n, scale, shift, relu, bf16):
    s64, h64 = np.abs(scale.astype(np.float64)), np.abs(shift.astype(np.float64))
    Bacc = C.gamma(2.0 * (np.asarray(n, np.float64) + 2.0)) * S if bf16 else C.bound(n, 2, S)
    E = s64 * Bacc + 2.0 * U * (np.abs(z) * s64 + h64) + 1e-30
    if not bf16:
        return E
    return E + B.BF16_EPS * (np.abs(reference(z, scale, shift, relu)) + E)


def accumulate(nbr, x, w, flip, descending):
    """The fp32 accumulator of a correct kernel: float32 products accumulated in float32 over the offsets in ascending or
    descending order (channels in the same order inside an offset), no final rounding.  -> (No, C_out) float32"""
    K, cin, cout = w.shape
    acc = np.zeros((nbr.shape[0], cout), np.float32)
    for k in (range(K - 1, -1, -1) if descending else range(K)):
        has = nbr[:, k] >= 0
        if not has.any():
            continue
        rows = x[nbr[has, k]]
        wk = w[K - 1 - k if flip else k]
        part = acc[has]
        for ci in (range(cin - 1, -1, -1) if descending else range(cin)):
            part = (part + (rows[:, ci:ci + 1] * wk[ci:ci + 1, :]).astype(np.float32)).astype(np.float32)
        acc[has] = part
    return acc


def emulate_epilogue(acc, scale, shift, relu, bf16):
    """fp32 fmaf through float64 (the product of two float32 is exact there), the NaN-passing ReLU with +0 for a negative value,
    and for bf16 the one rounding.  -> float32"""
    v = (acc.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    if relu:
        v = np.where(v > 0, v, np.where(np.isnan(v), v, np.float32(0.0))).astype(np.float32)
    return B.to_bf16(v) if bf16 else v
