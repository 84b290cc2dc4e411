"""Cases, float64 reference, bound and fp32 numpy emulation of the op-level tests of the inference Voxel-RoI pooling kernel
(mgar_voxel_roi_pool_eval_fwd / mgar_voxel_roi_pool_eval_bf16_fwd, csrc/voxel_roi_pool.hip), shared by
tests/test_voxel_roi_pool_eval_cpu.py (no kernel: the
bound is satisfiable, the cases exercise what they claim) and tests/test_voxel_roi_pool_eval_gpu.py.  Geometry, indices, features
and the position branch's parameters are voxel_roi_pool_cases.make_case's, unchanged; the float64 pooling is
torch_refs.voxel_roi_pool_ref(train=False).

Contract under test, per query m, channel c < C, output j < Co (include/mgar_ops.h):
    v = f + fmaf(w_pos[c] . r, ps_c, pb_c);  pooled_c = relu(max_s v);  z = sum_c W_out[j, c] pooled_c;
    out = act(fmaf(z, os_j, ob_j))                         (bf16: feats bf16, out rounded once)
with (ps, pb) the fp32 fold of the position BatchNorm's running statistics and affine (sparse_ops.fold_bn's formula in float64,
rounded once).  Reference: float64 on the fp32 operands (the bf16-rounded feats for bf16) with the UNfolded float64 BatchNorm.

Bound per element, u = 2^-24, a = |w0 rx| + |w1 ry| + |w2 rz| in float64:
    E_v    = 8 u (|f| + |ps_c| a + |pb_c|)     r, three products, two sums, the rounding of ps, fmaf, add: 7 roundings on the longest
                                               path; the rounding of pb, fmaf, add on |pb_c|
    E_pool = max_s E_v                         max and ReLU are 1-Lipschitz: no near-tie mask is needed for VALUES
    E_z    = sum_c |W_out[j,c]| E_pool[m,c] + gamma(2 (C + 1)) sum_c |W_out[j,c]| |pooled_ref[m,c]|
    E_out  = |os_j| E_z + 2 u (|z os_j| + |ob_j|)
    bf16:    E_out + 2^-8 (|ref| + E_out)
gamma(n) = torch_refs.gamma_u(n); its factor 2 would admit an MFMA summation."""
import functools

import numpy as np

import voxel_roi_pool_cases as VC

U = 2.0 ** -24
BF16_EPS = 2.0 ** -8

# (M, nsample, C), variant
CASES = [((180, 16, 16), None), ((2117, 16, 32), None), ((4999, 8, 12), None), ((333, 1, 1), None), ((130, 255, 5), None),
         ((5, 1, 3), None), ((1, 1, 2), None), (VC.ALL_EMPTY, "all_empty")]
assert all(s in VC.FULL_SIZES for s, v in CASES if v is None)
TINY = [(5, 1, 3), (1, 1, 2)]
# make_case's seed.  With seed 0 the single channel of (333, 1, 1) is clipped by the inner ReLU in 99 % of the queries: z is then
# one value almost everywhere and no out_shift puts 30-70 % of a channel's pre-activations below zero.  Seed 1 clips 36 %.
SEEDS = {(333, 1, 1): 1}
COUTS = [32, 7, 1]
PAD_F, PAD_OUT = 5, 3           # ld_f = C + PAD_F, ld_out = Co + PAD_OUT
SENTINEL = -77.0


def case_id(size, variant):
    return VC.size_id(size) + ("_" + variant if variant else "")


def to_bf16(a):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def fold(case):
    """(ps, pb) float32: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean scale, float64, rounded once"""
    g, b = case["gamma"].astype(np.float64), case["beta"].astype(np.float64)
    scale = g / np.sqrt(case["running_var"].astype(np.float64) + case["eps"])
    shift = b - case["running_mean"].astype(np.float64) * scale
    return scale.astype(np.float32), shift.astype(np.float32)


def act(v, relu):
    """float64 ReLU that passes a NaN (np.maximum does) -- or the identity"""
    return np.maximum(v, 0.0) if relu else v


@functools.lru_cache(maxsize=None)
def pooled_ref(size, variant, bf16):
    """-> (case dict with `feats` possibly bf16-rounded and ps / pb added, pooled (M, C) float64, E_pool (M, C) float64, empty
    (M,) bool).  Computed once per case and payload and shared: treat as read-only."""
    import torch
    import torch_refs as R
    case = dict(VC.make_case(*size, seed=SEEDS.get(size, 0), variant=variant))
    if bf16:
        case["feats"] = to_bf16(case["feats"])
    case["ps"], case["pb"] = fold(case)
    t = torch.from_numpy
    ref = R.voxel_roi_pool_ref(t(case["xyz"]), t(case["new_xyz"]), t(case["feats"]).double(), t(case["idx_raw"]), t(case["w_pos"]),
                               t(case["gamma"]), t(case["beta"]), case["eps"], False, t(case["running_mean"]), t(case["running_var"]))
    idx = case["idx_raw"].astype(np.int64)
    empty = idx[:, 0] == -1
    rows = np.where(empty[:, None], 0, np.maximum(idx, 0))
    f = np.abs(case["feats"].astype(np.float64))[rows] * (~empty)[:, None, None]                        # (M, ns, C)
    a = np.einsum("ck,msk->msc", np.abs(case["w_pos"].astype(np.float64)), np.abs(ref.r.numpy()))         # (M, ns, C)
    e_v = 8.0 * U * (f + np.abs(case["ps"].astype(np.float64)) * a + np.abs(case["pb"].astype(np.float64)))
    out = (case, ref.pooled.t().contiguous().numpy(), e_v.max(axis=1), empty)
    for v in list(case.values()) + list(out[1:]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def out_params(size, variant, bf16, co):
    """w_out (Co, C) standard normal / sqrt(C); out_scale of mixed sign over 10^U(-2, 2) with every fifth channel (from channel 1)
    exactly 0, as sparse_conv_affine_cases.affine_params; out_shift = minus a cut between two distinct values of the channel's
    z os, the one that leaves a share closest to clip(0.5 + 0.1 N(0, 1), 0.35, 0.65) of the pre-activations negative (pooled
    has an atom at 0, so a median would not do), and a standard normal where the scale is 0.
    -> (w_out, out_scale, out_shift, z float64 (M, Co))"""
    _, pooled, _, _ = pooled_ref(size, variant, bf16)
    c = size[2]
    rng = np.random.default_rng([11, size[0], size[1], c, co])
    w_out = (rng.standard_normal((co, c)) / np.sqrt(c)).astype(np.float32)
    scale = (rng.choice([-1.0, 1.0], co) * 10.0 ** rng.uniform(-2, 2, co)).astype(np.float32)
    scale[1::5] = 0.0
    z = pooled @ w_out.astype(np.float64).T
    zs = z * scale.astype(np.float64)
    g = rng.standard_normal(co)
    shift = g.copy()
    for j in np.nonzero(scale)[0]:
        vals = np.unique(zs[:, j])                                    # sorted, distinct
        cuts = np.concatenate([[vals[0] - 1.0], 0.5 * (vals[1:] + vals[:-1]), [vals[-1] + 1.0]])
        below = np.searchsorted(np.sort(zs[:, j]), cuts, side="left") / float(size[0])
        shift[j] = -cuts[np.argmin(np.abs(below - np.clip(0.5 + 0.1 * g[j], 0.35, 0.65)))]
    shift = shift.astype(np.float32)
    for v in (w_out, scale, shift, z):
        v.setflags(write=False)
    return w_out, scale, shift, z


def reference(size, variant, bf16, co, relu):
    """-> (ref (M, Co) float64, bound (M, Co) float64)"""
    _, pooled, e_pool, _ = pooled_ref(size, variant, bf16)
    import torch_refs as R
    w_out, scale, shift, z = out_params(size, variant, bf16, co)
    aw, s64, h64 = np.abs(w_out.astype(np.float64)), scale.astype(np.float64), shift.astype(np.float64)
    ref = act(z * s64 + h64, relu)
    e_z = e_pool @ aw.T + R.gamma_u(2.0 * (size[2] + 1)) * (np.abs(pooled) @ aw.T)
    e_out = np.abs(s64) * e_z + 2.0 * U * (np.abs(z * s64) + np.abs(h64))
    if bf16:
        e_out = e_out + BF16_EPS * (np.abs(ref) + e_out)
    return ref, e_out


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def emulate(size, variant, bf16, co, relu, order=None):
    """The chain in fp32 numpy as a correct kernel evaluates it: every product and sum rounded to float32, the two fmaf through
    float64 (a product of two float32 is exact there), the NaN-passing ReLUs, the sum over c in `order` (ascending by
    default), one rounding to bf16 at the end.  -> (M, Co) float32"""
    case, _, _, empty = pooled_ref(size, variant, bf16)
    w_out, scale, shift, _ = out_params(size, variant, bf16, co)
    idx = case["idx_raw"].astype(np.int64)
    rows = np.where(empty[:, None], 0, np.maximum(idx, 0))
    keep = (~empty)[:, None, None]
    r = (case["xyz"][rows] - case["new_xyz"][:, None, :]) * keep.astype(np.float32)                     # float32
    w = case["w_pos"]
    p = (r[:, :, None, 0] * w[None, None, :, 0] + r[:, :, None, 1] * w[None, None, :, 1]).astype(np.float32)
    p = (p + r[:, :, None, 2] * w[None, None, :, 2]).astype(np.float32)                                 # (M, ns, C)
    bn = _f32(p.astype(np.float64) * case["ps"].astype(np.float64) + case["pb"].astype(np.float64))
    v = (case["feats"][rows] * keep.astype(np.float32) + bn).astype(np.float32)
    pooled = np.maximum(v.max(axis=1), np.float32(0.0))                                                 # (M, C) float32
    order = range(size[2]) if order is None else order
    z = np.zeros((size[0], co), np.float32)
    for c in order:
        z = _f32(z.astype(np.float64) + pooled[:, c:c + 1].astype(np.float64) * w_out[None, :, c].astype(np.float64))
    o = _f32(z.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64))
    if relu:
        o = np.where(o > 0, o, np.where(np.isnan(o), o, np.float32(0.0))).astype(np.float32)
    return to_bf16(o) if bf16 else o
