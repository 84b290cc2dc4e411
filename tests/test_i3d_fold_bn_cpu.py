"""The eval-mode BatchNorm [+ ReLU] store of the dense I3D convolutions without a GPU: the four entry points are declared, exported
and bound with the header's prototypes; every refusal happens before any device call; sparse_ops.fold_bn on a BatchNorm3d against
a numpy float64 restatement, with its cache; the routing predicate Unit3D.eval_fold_plan; and the bounds of the device test are
satisfiable by a correct implementation."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import i3d_fold_bn_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K3, K3_BF = "mgar_conv3d_k3_fwd_affine", "mgar_conv3d_k3_bf16_fwd_affine"
STEM, STEM_BF = "mgar_stem_conv3d_fwd_affine", "mgar_stem_conv3d_bf16_fwd_affine"
NAMES = (K3, K3_BF, STEM, STEM_BF)
MGAR_OK, MGAR_EINVAL = 0, -1


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_four_symbols():
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
        assert name in _lib.exported_symbols()
        assert not name.endswith("_bf16") and name not in _lib.BF16_TWINS and name[:-5] not in _lib.BF16_TWINS
    assert len(_lib.BF16_TWINS) == 27
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    #       x  N Cin D H W  w Cout w_packed scale shift relu y y_batch_stride stream
    k3 = [P, I, I, I, I, I, P, I, P, P, P, I, P, LL, P]
    #         x  N T H W  w w_packed scale shift relu y stream
    stem = [P, I, I, I, I, P, P, P, P, I, P, P]
    for name, want in ((K3, k3), (K3_BF, k3), (STEM, stem), (STEM_BF, stem)):
        fn = _lib._fns[name]
        assert fn.restype is I and list(fn.argtypes) == want, name
    assert _lib.ABI_VERSION >= 20
    assert cdll.mgar_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("name", [K3, K3_BF])
def test_k3_entries_refuse_before_any_device_call(name):
    from multimodal_gar_amd import _lib
    fn = _lib._fns[name]
    one = ctypes.c_void_p(16)                      # non-null, 16-byte aligned, never dereferenced: every call below fails first
    cin = 8

    def call(N=2, Cin=cin, D=2, H=3, W=4, Cout=5, x=one, w=one, wp=one, scale=one, shift=one, y=one, stride=None):
        return fn(x, N, Cin, D, H, W, w, Cout, wp, scale, shift, 1, y, Cout * D * H * W if stride is None else stride, None)

    for bad in (dict(N=-1), dict(Cin=0), dict(Cout=0), dict(D=0), dict(H=0), dict(W=0)):
        assert call(**bad) == MGAR_EINVAL, bad
    assert call(W=5) == MGAR_EINVAL                                            # odd W
    assert call(Cin=7) == MGAR_EINVAL                                          # odd Cin
    if name == K3_BF:
        for c in (2, 4, 12):
            assert call(Cin=c) == MGAR_EINVAL, c                               # Cin % 8
    for k in ("x", "w", "wp", "scale", "shift", "y"):                          # each null pointer; scale and shift are both required
        assert call(**{k: None}) == MGAR_EINVAL, k
        assert b"null pointer" in _lib._cdll.mgar_last_error()
    for addr in ((4, 12, 20) if name == K3 else (1, 3, 17)):                   # a misaligned y: fp32 stores 8-byte pairs, bf16 2-byte elements
        assert call(y=ctypes.c_void_p(addr)) == MGAR_EINVAL, addr
        assert b"aligned" in _lib._cdll.mgar_last_error()
    assert call(stride=5 * 2 * 3 * 4 + 1) == MGAR_EINVAL                       # odd
    assert b"y_batch_stride" in _lib._cdll.mgar_last_error()
    assert call(stride=5 * 2 * 3 * 4 - 2) == MGAR_EINVAL                       # below Cout * D * H * W
    assert call(stride=0) == MGAR_EINVAL
    assert fn(None, 0, cin, 2, 3, 4, None, 5, None, None, None, 1, None, 0, None) == MGAR_OK     # nothing launched
    assert fn(None, 0, cin, 2, 3, 4, None, 5, None, None, None, 0, None, 120, None) == MGAR_OK
    assert call(N=0, W=5) == MGAR_EINVAL                                       # the shape rules hold for an empty launch too


@pytest.mark.parametrize("name", [STEM, STEM_BF])
def test_stem_entries_refuse_before_any_device_call(name):
    from multimodal_gar_amd import _lib
    fn = _lib._fns[name]
    one = ctypes.c_void_p(16)

    def call(N=1, T=2, H=10, W=8, x=one, w=one, wp=one, scale=one, shift=one, y=one):
        return fn(x, N, T, H, W, w, wp, scale, shift, 1, y, None)

    for bad in (dict(N=-1), dict(T=0), dict(H=0), dict(W=0)):
        assert call(**bad) == MGAR_EINVAL, bad
    for k in ("x", "w", "wp", "scale", "shift", "y"):
        assert call(**{k: None}) == MGAR_EINVAL, k
        assert b"null pointer" in _lib._cdll.mgar_last_error()
    assert call(N=70000) == MGAR_EINVAL and call(T=140000) == MGAR_EINVAL      # the plain entry's grid limits
    assert fn(None, 0, 2, 10, 8, None, None, None, None, 1, None, None) == MGAR_OK
    assert fn(None, 0, 3, 9, 10, None, None, None, None, 0, None, None) == MGAR_OK


# ---- fold_bn on a BatchNorm3d ---------------------------------------------------------------------------------------------------
def _bn3d(c, affine, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm3d(c, eps=1e-3, momentum=0.01, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 3.0)
        bn.running_var.copy_(torch.rand(c, generator=g) * 4.0 + 1e-4)
        if affine:
            bn.weight.copy_(torch.randn(c, generator=g))
            bn.bias.copy_(torch.randn(c, generator=g))
    return bn


def _fold_ref(bn):
    c = bn.num_features
    gamma = bn.weight.detach().numpy().astype(np.float64) if bn.affine else np.ones(c)
    beta = bn.bias.detach().numpy().astype(np.float64) if bn.affine else np.zeros(c)
    scale = gamma / np.sqrt(bn.running_var.numpy().astype(np.float64) + bn.eps)
    return scale, beta - bn.running_mean.numpy().astype(np.float64) * scale


def _within_one_ulp(got, want64):
    rounded = want64.astype(np.float32)
    return bool((np.abs(got.astype(np.float64) - rounded.astype(np.float64)) <= np.spacing(np.abs(rounded))).all())


@pytest.mark.parametrize("affine", [True, False])
def test_fold_bn_on_batchnorm3d_matches_the_float64_restatement_and_caches(affine):
    from multimodal_gar_amd import sparse_ops
    bn = _bn3d(37, affine, 3 + affine)
    scale, shift = sparse_ops.fold_bn(bn)
    assert scale.dtype == shift.dtype == torch.float32 and scale.shape == shift.shape == (37,)
    assert not scale.requires_grad and not shift.requires_grad
    want_scale, want_shift = _fold_ref(bn)
    assert _within_one_ulp(scale.numpy(), want_scale) and _within_one_ulp(shift.numpy(), want_shift)
    again = sparse_ops.fold_bn(bn)
    assert again[0] is scale and again[1] is shift                             # the same tensors: nothing computed
    with torch.no_grad():
        bn.running_mean.mul_(0.5)                                              # an in-place update: recomputed
    new = sparse_ops.fold_bn(bn)
    assert new[1] is not shift and not torch.equal(new[1], shift)
    assert _within_one_ulp(new[0].numpy(), _fold_ref(bn)[0]) and _within_one_ulp(new[1].numpy(), _fold_ref(bn)[1])
    assert sparse_ops.fold_bn(bn)[0] is new[0]
    assert "_mgar_folded" not in bn.state_dict() and len(bn.state_dict()) == (5 if affine else 3)


# ---- the routing predicate ------------------------------------------------------------------------------------------------------
def _like(shape, dtype=torch.float32, is_cuda=True, requires_grad=False, contiguous=True):
    """what eval_fold_plan reads of the input: nothing but attributes"""
    return types.SimpleNamespace(shape=torch.Size(shape), dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad,
                                 dim=lambda: len(shape), is_contiguous=lambda: contiguous)


def _input_of(unit, **kw):
    return _like((1, unit.conv3d.in_channels, 4, 12, 16), **kw)


def _frozen(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_eval_fold_plan_on_the_trunk(monkeypatch):
    """Every 7x7x7 / 3x3x3 unit of InceptionI3d('Mixed_4f') folds in eval mode under no_grad -- the stem, Conv3d_2c_3x3 and the 14
    branch units -- and no 1x1x1 unit does; in train mode none does."""
    from multimodal_gar_amd.model.backbone import InceptionI3d, Unit3D
    monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
    net = InceptionI3d(final_endpoint="Mixed_4f")
    net.build()
    net.eval()
    units = [m for m in net.modules() if isinstance(m, Unit3D)]
    big = [u for u in units if u._kernel_shape != (1, 1, 1)]
    assert len(big) == 16 and len(units) - len(big) == 1 + 4 * 7               # Conv3d_2b_1x1 + four 1x1x1 units per Mixed block
    with torch.no_grad():
        routes = [u.eval_fold_plan(_input_of(u)) for u in big]
        assert routes == ["stem"] + ["k3"] * 15
        assert [u.eval_fold_plan(_input_of(u, dtype=torch.bfloat16)) for u in big] == ["stem"] + ["k3_bf16"] * 15
        for u in units:
            if u._kernel_shape == (1, 1, 1):
                assert u.eval_fold_plan(_input_of(u)) is None and u.eval_fold_plan(_input_of(u, dtype=torch.bfloat16)) is None
        net.train()
        assert all(u.eval_fold_plan(_input_of(u)) is None for u in units)
        net.eval()
        monkeypatch.setattr(Unit3D, "fold_bn_eval", False)
        assert all(u.eval_fold_plan(_input_of(u)) is None for u in units)


def test_eval_fold_plan_conditions(monkeypatch):
    from multimodal_gar_amd.model.backbone import Unit3D
    monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
    k3 = Unit3D(16, 32, [3, 3, 3], name="k3").eval()
    stem = Unit3D(3, 64, [7, 7, 7], stride=(2, 2, 2), padding=(3, 3, 3), name="stem").eval()
    with torch.no_grad():
        assert k3.eval_fold_plan(_input_of(k3)) == "k3" and stem.eval_fold_plan(_input_of(stem)) == "stem"
        assert stem.eval_fold_plan(_like((1, 3, 3, 9, 11))) == "stem"                       # the stem's direct kernel takes any W
        for u in (k3, stem):
            x = _input_of(u)
            u.train()
            assert u.eval_fold_plan(x) is None                                              # train mode: batch statistics
            u.eval()
            u.bn.train()
            assert u.eval_fold_plan(x) is None                                              # only the BatchNorm's own flag counts
            u.bn.eval()
            assert u.eval_fold_plan(_input_of(u, is_cuda=False)) is None                    # host tensors
            assert u.eval_fold_plan(_input_of(u, dtype=torch.float16)) is None
            assert u.eval_fold_plan(_input_of(u, dtype=torch.float64)) is None
            u.emit_channels_last = True
            assert u.eval_fold_plan(x) is None                                              # the unit's BatchNorm writes NDHWC
            u.emit_channels_last = False
            monkeypatch.setattr(Unit3D, "fold_bn_eval", False)
            assert u.eval_fold_plan(x) is None                                              # the switch
            monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
            assert u.eval_fold_plan(x) is not None
        assert k3.eval_fold_plan(_like((1, 16, 4, 12, 15))) is None                         # odd W: the library convolution
        assert k3.eval_fold_plan(_like((1, 16, 4, 12, 16), contiguous=False)) is None       # (channels-last activations)
        assert Unit3D(12, 32, [3, 3, 3]).eval().eval_fold_plan(_like((1, 12, 4, 12, 16), dtype=torch.bfloat16)) is None   # Cin % 8
        k3.wino_kernel = False
        assert k3.eval_fold_plan(_input_of(k3)) is None                                     # no own kernel, nothing to fold into
        k3.wino_kernel = True
        # no running statistics; an activation that is not ReLU; no BatchNorm at all
        nostat = Unit3D(16, 32, [3, 3, 3]).eval()
        nostat.bn = nn.BatchNorm3d(32, eps=1e-3, track_running_stats=False).eval()
        assert nostat.eval_fold_plan(_input_of(nostat)) is None
        assert Unit3D(16, 32, [3, 3, 3], activation_fn=torch.tanh).eval().eval_fold_plan(_input_of(k3)) is None
        assert Unit3D(16, 32, [3, 3, 3], activation_fn=None).eval().eval_fold_plan(_input_of(k3)) == "k3"
        assert Unit3D(16, 32, [3, 3, 3], use_batch_norm=False).eval().eval_fold_plan(_input_of(k3)) is None
        assert Unit3D(16, 32, [3, 3, 3], use_bias=True).eval().eval_fold_plan(_input_of(k3)) is None
        assert Unit3D(16, 32, [3, 3, 3], stride=(1, 2, 2)).eval().eval_fold_plan(_input_of(k3)) is None
    # a gradient: grad mode on and a parameter (or the input) requiring one
    assert k3.eval_fold_plan(_input_of(k3)) is None
    _frozen(k3)
    assert k3.eval_fold_plan(_input_of(k3)) == "k3"
    assert k3.eval_fold_plan(_input_of(k3, requires_grad=True)) is None
    for p in (k3.bn.weight, k3.bn.bias, k3.conv3d.weight):
        p.requires_grad_(True)
        assert k3.eval_fold_plan(_input_of(k3)) is None, p.shape
        with torch.no_grad():
            assert k3.eval_fold_plan(_input_of(k3, requires_grad=True)) == "k3"
        p.requires_grad_(False)


def test_unit3d_host_routing_without_a_device(monkeypatch):
    """Unit3D.forward in eval mode makes ONE call of the route's affine entry and none of the BatchNorm kernels; it writes into
    `out` when that is an addressable channel slice and into a fresh tensor otherwise.  No device: L.call records names."""
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.model.backbone import Unit3D
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append((name, a)) or 0)
    monkeypatch.setattr(L, "raw", lambda name, *a: 64)
    monkeypatch.setattr(L, "dev_ptr", lambda t, dtype=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(L, "stream_of", lambda t: None)
    monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
    # (bn_ops._slice_stride wants a device tensor; its stride rules are its own tests' business)
    monkeypatch.setattr("multimodal_gar_amd.bn_ops._slice_stride", lambda out, like: out.stride(0) if out is not None else None)
    u = _frozen(Unit3D(16, 32, [3, 3, 3], name="k3")).eval()
    monkeypatch.setattr(u, "eval_fold_plan", lambda x: "k3_bf16" if x.dtype == torch.bfloat16 else "k3")   # (a host tensor stands in)
    for dtype, want in ((torch.float32, K3), (torch.bfloat16, K3_BF)):
        x = torch.zeros(2, 16, 2, 4, 6, dtype=dtype)
        del calls[:]
        y = u(x)
        assert [c[0] for c in calls] == [want] and y.shape == (2, 32, 2, 4, 6) and y.dtype == dtype
        assert calls[0][1][11] == 1 and calls[0][1][13] == 32 * 2 * 4 * 6                  # relu, the contiguous batch stride
        wide = torch.zeros(2, 56, 2, 4, 6, dtype=dtype)
        dst = wide[:, 8:40]
        del calls[:]
        r = u(x, out=dst)
        assert r is dst and [c[0] for c in calls] == [want]
        assert calls[0][1][12] == dst.data_ptr() and calls[0][1][13] == 56 * 2 * 4 * 6     # the slice's own batch stride


# ---- the device test's bounds ---------------------------------------------------------------------------------------------------
ALL = [("k3", s, False) for s in C.K3_FP32] + [("k3", s, True) for s in C.K3_BF16] + [("stem", s, s[4]) for s in C.STEM]


@pytest.mark.parametrize("kind,shape,bf16", ALL, ids=["%s-%s-%s" % (k, "x".join(str(int(v)) for v in s), "bf16" if b else "fp32") for k, s, b in ALL])
def test_bounds_are_satisfiable_by_a_correct_implementation(kind, shape, bf16):
    """The float64 convolution rounded to fp32 as the accumulator, fp32 fmaf via float64, the ReLU, one rounding: inside every bound
    of the device test on every case, with and without ReLU; the scale vector has a negative, a zero and a large entry and about
    half of the pre-activations are negative."""
    c = C.k3_case(shape, bf16) if kind == "k3" else C.stem_case(shape)
    z, scale, shift = c["z"], c["scale"], c["shift"]
    assert scale[0] < 0 and scale[1] == 0 and scale[2] == 1000.0
    pre = C.reference(z, scale, shift, 0)
    assert 0.2 <= (pre < 0).mean() <= 0.8
    z32 = z.astype(np.float32).astype(np.float64)
    for relu in (0, 1):
        got = C.emulate(z, None, scale, shift, relu, bf16).astype(np.float64)
        if relu:
            assert not np.signbit(got).any()
        if bf16:
            assert (np.abs(got - C.reference(z, scale, shift, relu)) <= C.bound_bf16(z, c["S"], c["n"], scale, shift, relu)).all()
        else:
            v64 = C.reference(z32, scale, shift, relu)
            assert (np.abs(got - v64) <= C.fma_bound(v64)).all()
            assert (np.abs(got - C.reference(z, scale, shift, relu)) <= C.truth_bound_fp32(z, scale, shift)).all()
