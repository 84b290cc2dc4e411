"""Shapes, operands, float64 references and bounds of the tests of the eval-mode BatchNorm [+ ReLU] store of the dense I3D
convolutions (mgar_conv3d_k3_fwd_affine, mgar_conv3d_k3_bf16_fwd_affine, mgar_stem_conv3d_fwd_affine,
mgar_stem_conv3d_bf16_fwd_affine), shared by tests/test_i3d_fold_bn_cpu.py and tests/test_i3d_fold_bn_gpu.py.

Contract under test, with acc the value the plain entry stores: v = fmaf(acc, scale[c], shift[c]); out = relu ? max(v, +0) with a
NaN passed through : v; a bf16 payload rounds out once.  References are float64 convolutions of the operands (the bf16-rounded
operands for bf16), computed once per case and shared: treat everything returned here as read-only.

Bounds:
  * fp32, against the plain entry's own output z (so only the epilogue is measured): one correctly rounded fp32 fma,
        |got - v64| <= (2^-24 + 2^-50) |v64| + 2^-149,   v64 = act(z64 * s64 + h64) in float64
    (2^-24 |v| is half an ulp of any normal result, 2^-149 covers the subnormal range, 2^-50 the float64 evaluation of v64 itself;
    the ReLU is exact);
  * fp32, against the float64 convolution: |scale_c| 5e-6 max|z| (the bound tests/test_conv3d_wino_gpu.py holds the plain kernels to,
    carried through the multiplication) + 2 * 2^-24 (|z scale_c| + |shift_c|) (the fma's rounding, factor 2 of slack);
  * bf16: sparse_conv_affine_cases.bound with n = 27 Cin (stem: 3 * 343) terms, S = conv(|x|, |w|), z the float64 convolution."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import sparse_conv_affine_cases as A
import sparse_conv_bf16_cases as B

U = 2.0 ** -24

# (n, cin, cout, d, h, w): the smallest shapes that reach every path of csrc/conv3d_wino.hip -- a tile larger than the image with one
# channel pair; 16-wide tiles with ragged H and W; 32-wide tiles with the 16-channel tail group (NMB = 1); N = 3 with a ragged last
# pair column; the 64-wide tile
K3_FP32 = ((1, 2, 48, 1, 5, 6), (1, 16, 32, 3, 9, 20), (1, 6, 208, 2, 23, 160), (3, 32, 96, 5, 17, 34), (1, 4, 64, 1, 4, 64))
# csrc/conv3d_bf16.hip: the same shapes with cin raised to a multiple of 8
K3_BF16 = tuple((n, -(-cin // 8) * 8, cout, d, h, w) for n, cin, cout, d, h, w in K3_FP32)
# (n, t, h, w, bf16) of the stem: minimal filtering (W % 4 == 0) on one tile and on N = 2, the direct fp32 kernel (W % 4 != 0), and the
# first two as bf16 payloads
STEM = ((1, 2, 10, 8, False), (2, 3, 12, 20, False), (1, 3, 9, 10, False), (1, 2, 10, 8, True), (2, 3, 12, 20, True))


def _bf16(t):
    return t.to(torch.bfloat16).float()


def affine_params(seed, z, channel_axis=1):
    """scale, shift (C) float32 for a float64 pre-BatchNorm tensor z: scale of mixed sign over 10^U(-2, 2), with a negative entry at
    channel 0, an exact zero at channel 1 (and every fifth from there) and a large one (1000) at channel 2; shift = half the channel's
    median |z scale| times a standard normal (a standard normal where that is 0): roughly half of the pre-activations are negative."""
    rng = np.random.default_rng(seed)
    c = z.shape[channel_axis]
    scale = (rng.choice([-1.0, 1.0], c) * 10.0 ** rng.uniform(-2, 2, c)).astype(np.float32)
    scale[0] = -abs(scale[0])
    scale[1::5] = 0.0
    scale[2] = 1000.0
    zc = np.moveaxis(z, channel_axis, 0).reshape(c, -1)
    spread = np.median(np.abs(zc * scale.astype(np.float64)[:, None]), axis=1)
    shift = (np.where(spread > 0, 0.5 * spread, 1.0) * rng.standard_normal(c)).astype(np.float32)
    return scale, shift


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def k3_operands(shape, bf16):
    """x (N, Cin, D, H, W) and w (Cout, Cin, 3, 3, 3) float32 tensors (bf16-valued for bf16): activations like the trunk's (post-ReLU,
    many zeros), weights centred -- the inputs tests/test_conv3d_wino_gpu.py holds the plain kernel to 5e-6 on"""
    n, cin, cout, d, h, w = shape
    g = torch.Generator().manual_seed(cin * 1000 + cout + w + (7 if bf16 else 0))
    x = torch.relu(torch.randn(n, cin, d, h, w, generator=g) + 0.3)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
    return (_bf16(x), _bf16(wt)) if bf16 else (x, wt)


def k3_conv64(x, wt):
    """float64 3x3x3 'same' convolution of float32 tensors -> (z, S = conv(|x|, |w|)) numpy float64"""
    z = F.conv3d(x.double(), wt.double(), None, 1, 1)
    S = F.conv3d(x.double().abs(), wt.double().abs(), None, 1, 1)
    return z.numpy(), S.numpy()


@functools.lru_cache(maxsize=None)
def k3_case(shape, bf16):
    """-> dict(x, w: float32 tensors; z, S: float64 (N, Cout, D, H, W); n: terms per output; scale, shift: float32 (Cout))"""
    x, wt = k3_operands(shape, bf16)
    z, S = k3_conv64(x, wt)
    scale, shift = affine_params(sum(shape) + 31 * bf16, z)
    return _freeze(dict(x=x, w=wt, z=z, S=S, n=27 * shape[1], scale=scale, shift=shift))


def stem_pads(t, h, w):
    """F.pad argument of the TF 'same' padding of a kernel-7, stride-2 convolution (model/backbone.py, _same_pad_1d)"""
    pads = []
    for size in (w, h, t):
        total = 5 if size % 2 == 0 else 6
        pads += [total // 2, total - total // 2]
    return pads


def stem_conv64(x, wt):
    t, h, w = x.shape[2:]
    z = F.conv3d(F.pad(x.double(), stem_pads(t, h, w)), wt.double(), stride=2)
    S = F.conv3d(F.pad(x.double().abs(), stem_pads(t, h, w)), wt.double().abs(), stride=2)
    return z.numpy(), S.numpy()


@functools.lru_cache(maxsize=None)
def stem_case(shape):
    """shape = (n, t, h, w, bf16) -> the dict of k3_case for the stem: x (N, 3, T, H, W), w (64, 3, 7, 7, 7)"""
    n, t, h, w, bf16 = shape
    g = torch.Generator().manual_seed(11 + 100 * t + h + w + (7 if bf16 else 0))
    x = torch.randn(n, 3, t, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, 7, generator=g) * (2.0 / 1029) ** 0.5
    if bf16:
        x, wt = _bf16(x), _bf16(wt)
    z, S = stem_conv64(x, wt)
    scale, shift = affine_params(5 + n + t + h + w + 31 * bf16, z)
    return _freeze(dict(x=x, w=wt, z=z, S=S, n=3 * 343, scale=scale, shift=shift))


def per_channel(v, ndim=5):
    """(C,) -> broadcastable against (N, C, ...) float64"""
    return np.asarray(v, np.float64).reshape((1, -1) + (1,) * (ndim - 2))


def reference(z, scale, shift, relu):
    """act(z * scale + shift) in float64 (a NaN passes the ReLU)"""
    return A.act(z * per_channel(scale, z.ndim) + per_channel(shift, z.ndim), relu)


def fma_bound(v64):
    """one correctly rounded fp32 fma of a value v64 evaluated in float64"""
    return (U + 2.0 ** -50) * np.abs(v64) + 2.0 ** -149


def truth_bound_fp32(z, scale, shift):
    s, h = np.abs(per_channel(scale, z.ndim)), np.abs(per_channel(shift, z.ndim))
    finite = np.abs(z[np.isfinite(z)])
    return s * 5e-6 * (finite.max() if finite.size else 0.0) + 2.0 * U * (np.abs(z) * s + h)


def bound_bf16(z, S, n, scale, shift, relu):
    return A.bound(z, S, n, per_channel(scale, z.ndim), per_channel(shift, z.ndim), relu, True)


def emulate(z, S_unused, scale, shift, relu, bf16):
    """what a correct kernel stores for the accumulator z rounded to fp32: fmaf through float64 (the product of two float32 is exact
    there; the one addition is then rounded to float32 -- double rounding can differ from fmaf by at most the 2^-50 term of
    fma_bound), the NaN-passing ReLU with +0 for a negative value, and for bf16 the one rounding.  -> float32"""
    acc = z.astype(np.float32)
    return A.emulate_epilogue(acc, per_channel(scale, z.ndim).astype(np.float32), per_channel(shift, z.ndim).astype(np.float32), relu, bf16)


def to_bf16(a):
    return B.to_bf16(a)
