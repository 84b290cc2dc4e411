"""Value cases, bound and numpy emulation of the op-level tests of csrc/sparse_conv_bf16.hip, shared by
tests/test_sparse_conv_bf16_cpu.py (the bound is satisfiable: no kernel involved) and tests/test_sparse_conv_bf16_gpu.py.
Tables, inputs and the float64 reference come from tests/sparse_conv_cases.py unchanged.

Operands are rounded to bf16 with torch; the float64 reference is gather_gemm_ref on the ROUNDED x and w, so the comparison
sees the kernel's own error only.  Per element
    |got - ref| <= B + 2^-8 (|ref| + B) + 1e-30,   B = gamma(2 (n + 2)) S
with S = sum |x| |w| over the element's products, n their number and gamma as in the cases module (u = 2^-24): B bounds the
fp32 accumulation of the exact products in any order -- the factor 2 allows an accumulator that truncates instead of rounding
to nearest, the MFMA's internal rounding being undocumented -- and 2^-8 is the one final rounding to bf16 (8 significand bits,
nearest even: unit roundoff 2^-8) of a value within B of ref.  A correct kernel therefore uses up to all of the bound on some
element: the rounding term is attained, not estimated."""
import functools

import numpy as np
import torch

import sparse_conv_cases as C

TRUNK_PLANS = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128))      # VoxelBackBone8x after conv_input
PLANS = TRUNK_PLANS + ((128, 128), (48, 40), (16, 1), (112, 33))
ROWS_PLANS = ((16, 16), (64, 128))
SMALL_K_PLANS = ((16, 16), (48, 40))
BF16_EPS = 2.0 ** -8


def to_bf16(a):
    """float32 array -> the same values rounded to bf16 (nearest even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def bound(ref, S, n):
    B = C.gamma(2.0 * (np.asarray(n, np.float64) + 2.0)) * S
    return B + BF16_EPS * (np.abs(ref) + B) + 1e-30


@functools.lru_cache(maxsize=None)
def subm_table(n):
    """nbr of the submanifold k3 rulebook over exactly n sites (reference), shared and left unchanged"""
    nbr = C.rulebook_ref(C.rows_case(n), C.ROWS_GRID, 3, 1, 1, True)[2]
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def main_table():
    nbr = C.main_table()[0]
    nbr.setflags(write=False)
    return nbr


@functools.lru_cache(maxsize=None)
def alternate_tiles_table():
    nbr = C.builder_tables()["alternate_tiles"]
    nbr.setflags(write=False)
    return nbr


def value_cases():
    """name -> (table, C_in, C_out, flip_k, seed)"""
    out = {}
    for cin, cout in PLANS:
        out["plan_%dx%d" % (cin, cout)] = (subm_table(C.PLAN_ROWS), cin, cout, 0, 1000 + 131 * cin + cout)
    for n in C.ROWS:
        for cin, cout in ROWS_PLANS:
            out["rows_%d_%dx%d" % (n, cin, cout)] = (subm_table(n), cin, cout, 0, 2000 + 7 * n + cin)
    for K in C.SMALL_K:
        for cin, cout in SMALL_K_PLANS:
            out["small_k%d_%dx%d" % (K, cin, cout)] = (C.small_table(K), cin, cout, 0, 3000 + 11 * K + cin)
    out["flip_32x64"] = (subm_table(C.PLAN_ROWS), 32, 64, 1, 4000)
    out["alternate_tiles_32x32"] = (alternate_tiles_table(), 32, 32, 0, 5000)
    out["main_64x64"] = (main_table(), 64, 64, 0, 6000)
    return out


def operands(name):
    """-> nbr, x (rows, C_in) and w (K, C_in, C_out) float32 holding bf16 values, flip_k: wide_range features (an error in a
    small-magnitude channel cannot hide under the global maximum) and weights(...), both rounded to bf16 with torch."""
    nbr, cin, cout, flip, seed = value_cases()[name]
    rng = np.random.default_rng(seed)
    n_src = int(nbr.max()) + 1 if nbr.size and nbr.max() >= 0 else 1
    x = to_bf16(C.wide_range(rng, (max(n_src, nbr.shape[0]), cin)))
    w = to_bf16(C.weights(rng, nbr.shape[1], cin, cout))
    return nbr, x, w, flip


def emulate(nbr, x, w, flip, descending):
    """A correct implementation in numpy: float32 products of the rounded operands (exact: 8 x 8 significand bits), accumulated in
    float32 over the offsets in ascending or descending order (channels in order inside an offset), ONE rounding to bf16 at the
    end.  -> (No, C_out) float32 holding bf16 values."""
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
            part = (part + rows[:, ci:ci + 1] * wk[ci:ci + 1, :]).astype(np.float32)
        acc[has] = part
    return to_bf16(acc)
