"""Cases, operands, float64 reference and bounds shared by tests/test_conv1x1_bf16_cpu.py and tests/test_conv1x1_bf16_gpu.py for
mgar_conv1x1_bf16_fwd / mgar_conv1x1_bf16_fwd_affine (csrc/pointwise_wide_bf16.hip).

The kernel's contract (include/mgar_ops.h):
    w~[o,i]    = bf16(w[o,i])
    acc[n,o,p] = sum_i w~[o,i] x[n,i,p]                  fp32, exact products
    plain:  y = bf16(acc)            affine:  y = bf16(relu?(fmaf(acc, scale[o], shift[o])))
Operands as tests/i3d_fold_bn_cases.k3_operands: post-ReLU activations, centred weights of variance 2 / Cin, bf16-valued; scale and
shift from i3d_fold_bn_cases.affine_params (a negative, a zero and a 1000x channel).  The reference is the float64 product of the
rounded operands.  No new tolerance: the plain entry is held to pointwise_bf16_cases.reference (B + 2^-8 (|ref| + B),
B = gamma(2 (Cin + 2)) S), the affine entry to sparse_conv_affine_cases.bound(z, S, n = Cin, scale, shift, relu, bf16 = True).
Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch

import i3d_fold_bn_cases as F
import pointwise_bf16_cases as PC
import sparse_conv_affine_cases as A

BF = torch.bfloat16

# (N, Cin, Cout, P): the smallest shapes that reach every path
CASES = (
    (1, 8, 8, 4),           # one column quad, half a k-step
    (1, 64, 64, 132),       # a ragged second tile
    (1, 40, 24, 516),       # Cin not a multiple of 16, Cout 24
    (2, 192, 96, 96),       # three 32-row blocks
    (2, 480, 16, 180),      # half a row block, 30 k-steps
    (3, 528, 256, 260),     # the widest unit up to Mixed_4f; tiles straddle samples
    (2, 832, 384, 8),       # Mixed_5c's largest, P smaller than a tile
)


def case_id(case):
    return "x".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _drawn(case):
    n, cin, cout, p = case
    g = torch.Generator().manual_seed(cin * 1000 + cout + p)
    x = torch.relu(torch.randn(n, cin, p, generator=g) + 0.3)
    w = torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5
    return x.to(BF).float(), w


def operands(case):
    """-> (x (N, Cin, P), w (Cout, Cin)) float32 tensors holding bf16 values"""
    x, w = _drawn(case)
    return x, w.to(BF).float()


def unrounded_weight(case):
    """the fp32 weight the bf16-valued one of operands() was rounded from (what a kernel that forgets the rounding multiplies)"""
    return _drawn(case)[1]


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> dict: x, w (float32 tensors); ref, bound (float64 tensors, the plain entry); z, S (float64 numpy, (N, Cout, P)); scale,
    shift (float32 numpy (Cout)).  Shared: callers must not modify it."""
    x, w = operands(case)
    ref, bound = PC.reference(x, w)
    z = ref.numpy()
    S = torch.einsum("oi,bip->bop", w.double().abs(), x.double().abs()).numpy()
    scale, shift = F.affine_params(sum(case), z)
    for a in (z, S, scale, shift):
        a.setflags(write=False)
    return dict(x=x, w=w, ref=ref, bound=bound, z=z, S=S, scale=scale, shift=shift)


def per_channel(v):
    return np.asarray(v).reshape(1, -1, 1)


def affine_reference(case, relu):
    """-> (float64 reference, bound) of the affine entry, numpy (N, Cout, P)"""
    e = expected(case)
    sc, sh = per_channel(e["scale"]), per_channel(e["shift"])
    return A.reference(e["z"], sc, sh, relu), A.bound(e["z"], e["S"], case[1], sc, sh, relu, True)


def share(y, ref, bound):
    """largest |y - ref| / bound over the elements (numpy float64; every bound here is > 0)"""
    return float((np.abs(np.asarray(y, np.float64) - ref) / bound).max())


def plain_share(y, case):
    e = expected(case)
    return PC.share_of_bound(y, e["ref"], e["bound"])


def affine_share(y, case, relu):
    ref, bound = affine_reference(case, relu)
    return share(y, ref, bound)
