"""Cases, float64 reference and per-element bound of the op-level tests of the inference non-local kernel
(mgar_nonlocal_dot_eval_fwd / mgar_nonlocal_dot_eval_bf16_fwd, csrc/nonlocal_eval.hip), shared by tests/test_nonlocal_eval_cpu.py
(no kernel: the reference is checked against the kernel's own algebra) and tests/test_nonlocal_eval_gpu.py.

Contract under test, per sample (include/mgar_ops.h), x a (C, P) matrix:
    [T; Phi; G] = W_tpg x + b_tpg;   S = G Phi^T / P;   Y = S T;   z = fmaf(W_z Y + b_z, scale, shift) + x
with (scale, shift) the fp32 fold of the BatchNorm's running statistics and affine (float64, rounded once), 1 and 0 for a block
without one.  Reference: float64 on the fp32 operands (the bf16-rounded x for bf16) of the LITERAL formula of NLBlockND.forward --
the (P, P) matrix f = theta^T phi / P, y = f g^T, W_z, the UNfolded eval-mode BatchNorm, + x.

Bound per element: mag = the same chain with every operand replaced by its absolute value (non-negative arithmetic is
associative, so one mag covers both summation orders);
    bound = K 2^-24 mag,   K = C + P + 2 Ci + 8     the longest chain of dependent fp32 roundings (the standard gamma_n bound)
    bf16:   bound + 2^-8 |ref|                      one rounding to nearest even, doubled for the power-of-two boundary, as in
                                                    voxel_roi_pool_eval_cases.py
Parameters come from tests/golden/param_fill.fill_deterministic on an NLBlockND(C, Ci, mode='dot', dimension=1)."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from param_fill import fill_deterministic  # noqa: E402

U = 2.0 ** -24
BF16_EPS = 2.0 ** -8

# (n, C, Ci, P)
CASES = [(2, 832, 104, 25),     # the RGB model shape
         (3, 96, 12, 216),      # the LiDAR model shape
         (3, 32, 4, 25),        # golden fixture size (nl2d)
         (2, 24, 3, 216),       # golden fixture size (nl3d)
         (1, 5, 1, 1),          # degenerate
         (2, 8, 2, 33),         # one past a 32-wide tile
         (4, 7, 3, 256),        # odd channel counts at the largest supported P
         (300, 8, 2, 9)]        # more samples than a grid cap or grid-stride indexing would take in one wave of workgroups


def case_id(case):
    return "n%d_C%d_Ci%d_P%d" % case


def to_bf16(a):
    """float32 -> the nearest bf16 value (ties to even), as float32; a NaN stays a NaN"""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return np.where(np.isnan(a), a, b.astype(np.uint32).view(np.float32).reshape(a.shape))


def make_block(case, bn_layer, seed=3):
    """NLBlockND(C, Ci, mode='dot', dimension=1) with deterministic parameters and perturbed running statistics, in eval mode"""
    from multimodal_gar_amd.model.backbone import NLBlockND
    _, c, ci, _ = case
    return fill_deterministic(NLBlockND(c, ci, mode='dot', dimension=1, bn_layer=bn_layer), seed=seed).eval()


@functools.lru_cache(maxsize=None)
def params(case, bn_layer):
    """The block's parameters as numpy float32 (read-only): w_theta, b_theta, ... and the kernel's six arrays."""
    blk = make_block(case, bn_layer)
    _, c, ci, _ = case
    g = lambda t: t.detach().numpy().astype(np.float32)     # noqa: E731
    p = {k: g(getattr(blk, k).weight).reshape(ci, c) for k in ("theta", "phi", "g")}
    p.update({"b_" + k: g(getattr(blk, k).bias) for k in ("theta", "phi", "g")})
    conv_z = blk.W_z[0] if bn_layer else blk.W_z
    p["w_z"], p["b_z"] = g(conv_z.weight).reshape(c, ci), g(conv_z.bias)
    if bn_layer:
        bn = blk.W_z[1]
        p.update(gamma=g(bn.weight), beta=g(bn.bias), mean=g(bn.running_mean), var=g(bn.running_var), eps=float(bn.eps))
        scale = p["gamma"].astype(np.float64) / np.sqrt(p["var"].astype(np.float64) + p["eps"])
        shift = p["beta"].astype(np.float64) - p["mean"].astype(np.float64) * scale
        p["scale"], p["shift"] = scale.astype(np.float32), shift.astype(np.float32)
    else:
        p["scale"], p["shift"] = np.ones(c, np.float32), np.zeros(c, np.float32)
    p["w_tpg"] = np.concatenate([p["theta"], p["phi"], p["g"]])
    p["b_tpg"] = np.concatenate([p["b_theta"], p["b_phi"], p["b_g"]])
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def make_x(case, bf16=False):
    """x (n, C, P) float32, standard normal, seeded by the case (bf16: rounded to bf16 values); read-only"""
    n, c, _, p = case
    x = np.random.default_rng([7, n, c, p]).standard_normal((n, c, p)).astype(np.float32)
    x = to_bf16(x) if bf16 else x
    x.setflags(write=False)
    return x


def _chain(p, x, absolute):
    """The literal formula in float64 on (n, C, P) x.  absolute: every operand replaced by its absolute value."""
    a = np.abs if absolute else (lambda v: v)
    f64 = lambda v: a(np.asarray(v, np.float64))                                           # noqa: E731
    x = f64(x)
    proj = lambda w, b: np.einsum("ic,ncp->nip", f64(p[w]), x) + f64(p[b])[None, :, None]   # noqa: E731
    theta, phi, g = proj("theta", "b_theta"), proj("phi", "b_phi"), proj("g", "b_g")       # (n, Ci, P)
    f = np.einsum("nip,niq->npq", theta, phi) / x.shape[2]                                  # (n, P, P)
    y = np.einsum("npq,niq->nip", f, g)                                                     # (n, Ci, P)
    w = np.einsum("ci,nip->ncp", f64(p["w_z"]), y) + f64(p["b_z"])[None, :, None]
    if "gamma" in p:
        inv = 1.0 / np.sqrt(np.asarray(p["var"], np.float64) + p["eps"])
        mean = f64(p["mean"]) if absolute else -f64(p["mean"])
        w = (w + mean[None, :, None]) * (f64(p["gamma"]) * inv)[None, :, None] + f64(p["beta"])[None, :, None]
    return w + x


def reference_of(case, bn_layer, x, bf16=False):
    """-> (ref, bound), float64 (n, C, P), for the given x (already bf16-rounded for bf16)"""
    p = params(case, bn_layer)
    _, c, ci, pp = case
    with np.errstate(invalid="ignore"):
        ref, mag = _chain(p, x, False), _chain(p, x, True)
    bound = (c + pp + 2 * ci + 8) * U * mag
    if bf16:
        bound = bound + BF16_EPS * np.abs(ref)
    return ref, bound


@functools.lru_cache(maxsize=None)
def reference(case, bn_layer, bf16):
    """reference_of on make_x, computed once and shared: treat as read-only"""
    ref, bound = reference_of(case, bn_layer, make_x(case, bf16), bf16)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def factored(case, bn_layer, x):
    """The kernel's algebra in float64: S = G Phi^T / P, Y = S T, the FOLDED affine map in float64 -> (n, C, P)"""
    p = params(case, bn_layer)
    x = np.asarray(x, np.float64)
    tpg = np.einsum("ic,ncp->nip", p["w_tpg"].astype(np.float64), x) + p["b_tpg"].astype(np.float64)[None, :, None]
    ci = case[2]
    t, phi, g = tpg[:, :ci], tpg[:, ci:2 * ci], tpg[:, 2 * ci:]
    s = np.einsum("njp,nip->nji", g, phi) / x.shape[2]
    y = np.einsum("nji,nip->njp", s, t)
    w = np.einsum("ci,nip->ncp", p["w_z"].astype(np.float64), y) + p["b_z"].astype(np.float64)[None, :, None]
    if "gamma" in p:
        scale = p["gamma"].astype(np.float64) / np.sqrt(p["var"].astype(np.float64) + p["eps"])
        shift = p["beta"].astype(np.float64) - p["mean"].astype(np.float64) * scale
    else:
        scale, shift = np.ones(case[1]), np.zeros(case[1])
    return w * scale[None, :, None] + shift[None, :, None] + x
