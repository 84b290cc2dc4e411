"""The inference Voxel-RoI pooling route without a GPU: the two entry points (mgar_voxel_roi_pool_eval_fwd,
mgar_voxel_roi_pool_eval_bf16_fwd) are declared,
exported and bound with the header's prototypes and have their timer row; every refusal happens before any device call; the bound
of the device test is satisfiable by a correct fp32 evaluation and the cases exercise what they claim (both decided from the
float64 reference alone); the folded parameters of the host route against float64 eval-mode Conv + BatchNorm, with their cache; and
the routing predicate voxel_pool_modules.eval_fuse_plan."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import voxel_roi_pool_eval_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16 = "mgar_voxel_roi_pool_eval_fwd", "mgar_voxel_roi_pool_eval_bf16_fwd"
MGAR_OK, MGAR_EINVAL, MGAR_EUNSUPPORTED = 0, -1, -3
CASE_IDS = [E.case_id(s, v) for s, v in E.CASES]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_symbols():
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    I, P = ctypes.c_int, ctypes.c_void_p
    #      M ns C Co xyz new_xyz feats ld_f idx w_pos ps pb w_out os ob relu out ld_out stream
    want = [I, I, I, I, P, P, P, I, P, P, P, P, P, P, P, I, P, I, P]
    for name in (FP32, BF16):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
        assert name in _lib.exported_symbols()
        assert _lib._fns[name].restype is I and list(_lib._fns[name].argtypes) == want, name
    # called by name: neither is in the table of `_bf16` payload twins, whose size existing tests pin
    assert FP32 not in _lib.BF16_TWINS and not BF16.endswith("_bf16") and BF16[:-5] not in _lib.BF16_TWINS
    assert _lib.ABI_VERSION >= 19
    assert cdll.mgar_abi_version() == _lib.ABI_VERSION


def test_timer_row_and_source_map():
    from multimodal_gar_amd import _lib, op_timer
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert names[-1] == "voxel_roi_pool_eval" and len(set(names)) == len(names)      # appended: earlier ids keep their rows
    assert "voxel_roi_pool_fwd" in names
    assert op_timer.KERNEL_SOURCES.get("voxel_roi_pool_eval") == "voxel_roi_pool.hip"


@pytest.mark.parametrize("name", [FP32, BF16])
def test_entries_refuse_before_any_device_call(name):
    from multimodal_gar_amd import _lib
    fn = _lib._fns[name]
    one = ctypes.c_void_p(16)                      # non-null, aligned, never dereferenced: every call below fails first

    def call(M=5, ns=16, C=32, Co=32, ld_f=32, ld_out=32, ptrs=None):
        p = ptrs or [one] * 11                     # xyz new_xyz feats idx w_pos ps pb w_out os ob out
        return fn(M, ns, C, Co, p[0], p[1], p[2], ld_f, p[3], p[4], p[5], p[6], p[7], p[8], p[9], 1, p[10], ld_out, None)

    for C, Co in ((33, 32), (32, 33), (48, 48), (64, 7)):
        for M in (5, 0):                           # the plan rules hold for an empty launch too
            assert call(M=M, C=C, Co=Co, ld_f=64, ld_out=64) == MGAR_EUNSUPPORTED, (M, C, Co)
    for kw in (dict(M=-1), dict(ns=0), dict(ns=256), dict(ns=-3), dict(C=0), dict(Co=0), dict(C=-1), dict(ld_f=31),
               dict(ld_out=31), dict(C=5, Co=7, ld_f=4, ld_out=7), dict(C=5, Co=7, ld_f=5, ld_out=6)):
        assert call(**kw) == MGAR_EINVAL, kw
        assert b"bad sizes" in _lib._cdll.mgar_last_error()
    for k in range(11):                            # each null pointer with M > 0: every parameter vector is required
        p = [one] * 11
        p[k] = None
        assert call(ptrs=p) == MGAR_EINVAL, k
        assert b"null pointer" in _lib._cdll.mgar_last_error()
    assert call(M=0, ptrs=[None] * 11) == MGAR_OK                      # nothing launched
    assert call(M=0, ns=255, C=1, Co=1, ld_f=1, ld_out=1, ptrs=[None] * 11) == MGAR_OK
    assert call(C=5, Co=7, ld_f=5, ld_out=7, M=0, ptrs=[None] * 11) == MGAR_OK


# ---- the device test's bound and cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size,variant", E.CASES, ids=CASE_IDS)
def test_bound_is_satisfiable_by_a_correct_implementation(size, variant, bf16):
    """The fp32 numpy emulation of the chain, summed over c ascending and in a permuted order, stays inside the bound on every
    case, Co and activation."""
    worst = 0.0
    for co in E.COUTS:
        perm = np.random.default_rng([5, size[2], co]).permutation(size[2])
        for relu in (0, 1):
            ref, lim = E.reference(size, variant, bf16, co, relu)
            assert np.isfinite(ref).all() and (lim > 0).all()
            for order in (None, perm):
                got = E.emulate(size, variant, bf16, co, relu, order).astype(np.float64)
                used = float((np.abs(got - ref) / lim).max())
                worst = max(worst, used)
                assert used <= 1.0, (size, variant, co, relu, order is not None, used)
                if relu:
                    assert (got >= 0).all() and not np.signbit(got).any()
    print("%s %s: max err / bound = %.3f" % (E.case_id(size, variant), "bf16" if bf16 else "fp32", worst))


@pytest.mark.parametrize("size,variant", E.CASES, ids=CASE_IDS)
def test_cases_exercise_what_they_claim(size, variant):
    case, pooled, e_pool, empty = E.pooled_ref(size, variant, False)
    m, ns, c = size
    assert pooled.shape == (m, c) and e_pool.shape == (m, c) and (pooled >= 0).all()
    if variant == "all_empty":
        assert empty.all()
        want = np.maximum(case["pb"].astype(np.float64), 0.0)
        assert np.allclose(pooled, np.broadcast_to(want, pooled.shape), rtol=1e-6, atol=1e-7)   # pb is the fp32 fold
    elif size not in E.TINY:
        assert empty.any() and not empty.all()
    if ns == 1:                                    # one candidate: the inner ReLU alone decides
        assert (pooled == 0).mean() >= 0.10, (pooled == 0).mean()
    if m >= 180:
        for co in E.COUTS:
            w_out, scale, shift, z = E.out_params(size, variant, False, co)
            pre = z * scale.astype(np.float64) + shift.astype(np.float64)
            assert 0.3 <= (pre < 0).mean() <= 0.7, (co, (pre < 0).mean())
    w_out, scale, shift, z = E.out_params(size, variant, False, 32)
    assert (scale == 0).any() and (scale > 0).any() and (scale < 0).any()
    mags = np.abs(scale[scale != 0])
    assert mags.max() / mags.min() > 100


def test_the_bound_is_not_met_by_construction():
    """Ascending and permuted summation differ somewhere, and a dropped inner ReLU or an outer ReLU in front of the affine map
    leaves the bound."""
    size, variant = (180, 16, 16), None
    ref, lim = E.reference(size, variant, False, 32, 1)
    up = E.emulate(size, variant, False, 32, 1)
    perm = E.emulate(size, variant, False, 32, 1, np.random.default_rng(1).permutation(16))
    assert not np.array_equal(up, perm)
    w_out, scale, shift, z = E.out_params(size, variant, False, 32)
    wrong = np.maximum(z, 0.0) * scale.astype(np.float64) + shift.astype(np.float64)          # ReLU before the affine map
    assert (np.abs(wrong - ref) / lim).max() > 1.0


# ---- the folded parameters ------------------------------------------------------------------------------------------------------
def _bn(kind, c, affine, seed):
    g = torch.Generator().manual_seed(seed)
    bn = kind(c, eps=1e-3, momentum=0.01, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 2.0)
        bn.running_var.copy_(torch.rand(c, generator=g) * 4.0 + 1e-3)
        if affine:
            bn.weight.copy_(torch.randn(c, generator=g))
            bn.bias.copy_(torch.randn(c, generator=g))
    return bn


def _restate(conv, bn):
    """numpy float64: eval-mode conv + BatchNorm as y = x W'^T + b' -> (scale, W', b')"""
    c = bn.num_features
    w = conv.weight.detach().numpy().astype(np.float64).reshape(conv.out_channels, conv.in_channels)
    gamma = bn.weight.detach().numpy().astype(np.float64) if bn.affine else np.ones(c)
    beta = bn.bias.detach().numpy().astype(np.float64) if bn.affine else np.zeros(c)
    scale = gamma / np.sqrt(bn.running_var.numpy().astype(np.float64) + bn.eps)
    shift = beta - bn.running_mean.numpy().astype(np.float64) * scale
    if conv.bias is not None:
        shift = shift + conv.bias.detach().numpy().astype(np.float64) * scale
    return scale, scale[:, None] * w, shift


def _close(got, want, roundings):
    return bool((np.abs(got.astype(np.float64) - want) <= roundings * 2.0 ** -24 * np.abs(want) + 1e-38).all())


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no_affine"])
@pytest.mark.parametrize("bias", [False, True], ids=["no_bias", "conv_bias"])
def test_folded_parameters_reproduce_eval_mode_conv_and_batchnorm(affine, bias):
    """Two steps.  (1) The float64 restatement y = x W'^T + b' IS eval-mode Conv + BatchNorm: against torch's own float64 modules
    to 1e-12 relative, for mlps_in (Conv1d), mlps_pos (Conv2d) and mlps_out.  (2) What the host route hands the kernels is that
    restatement rounded to fp32: fold_bn's scale / shift once, W' twice (the fp32 scale, then the product formed in float64)."""
    from multimodal_gar_amd import sparse_ops
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    g = torch.Generator().manual_seed(21)
    for conv, bn, x in ((nn.Conv1d(16, 32, 1, bias=bias), _bn(nn.BatchNorm1d, 32, affine, 1), torch.randn(1, 16, 50, generator=g)),
                        (nn.Conv2d(3, 32, 1, bias=bias), _bn(nn.BatchNorm2d, 32, affine, 2), torch.randn(1, 3, 10, 5, generator=g)),
                        (nn.Conv1d(32, 7, 1, bias=bias), _bn(nn.BatchNorm1d, 7, affine, 3), torch.randn(1, 32, 50, generator=g))):
        if bias:
            with torch.no_grad():
                conv.bias.copy_(torch.randn(conv.out_channels, generator=g))
        scale, w_f, b_f = _restate(conv, bn)
        with torch.no_grad():
            import copy
            truth = copy.deepcopy(bn).double()(copy.deepcopy(conv).double()(x.double())).flatten(2)[0].numpy()   # (C_out, P)
        rows = x.double().flatten(2)[0].numpy().T                                                                # (P, C_in)
        mine = (rows @ w_f.T + b_f).T
        assert np.abs(mine - truth).max() <= 1e-12 * np.abs(truth).max()
        s32, b32 = sparse_ops.fold_bn(bn, conv.bias)
        assert _close(s32.numpy(), scale, 1.0) and _close(b32.numpy(), b_f, 1.0)
        if isinstance(conv, nn.Conv1d) and conv.in_channels == 16:
            folded = V.folded_mlp_in(conv, bn)
            w32, bias32 = folded[torch.float32]
            assert w32.dtype == torch.float32 and tuple(w32.shape) == (32, 16) and w32.is_contiguous() and not w32.requires_grad
            assert _close(w32.numpy(), w_f, 2.0) and bias32 is b32
            w16, bias16 = folded[torch.bfloat16]
            assert w16.dtype == bias16.dtype == torch.bfloat16
            assert torch.equal(w16, w32.to(torch.bfloat16)) and torch.equal(bias16, b32.to(torch.bfloat16))


def test_folded_mlp_in_cache_follows_versions():
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    conv, bn = nn.Conv1d(16, 32, 1, bias=False), _bn(nn.BatchNorm1d, 32, True, 4)
    a = V.folded_mlp_in(conv, bn)
    assert V.folded_mlp_in(conv, bn) is a                                     # the same tensors: nothing computed
    with torch.no_grad():
        conv.weight.mul_(2.0)
    b = V.folded_mlp_in(conv, bn)
    assert b is not a and torch.equal(b[torch.float32][0], a[torch.float32][0] * 2.0)
    assert V.folded_mlp_in(conv, bn) is b
    with torch.no_grad():
        bn.running_var.add_(0.5)
    c = V.folded_mlp_in(conv, bn)
    assert c is not b and _close(c[torch.float32][0].numpy(), _restate(conv, bn)[1], 2.0)
    assert V.folded_mlp_in(conv, bn) is c
    bn.load_state_dict(_bn(nn.BatchNorm1d, 32, True, 5).state_dict())
    d = V.folded_mlp_in(conv, bn)
    assert d is not c and _close(d[torch.float32][0].numpy(), _restate(conv, bn)[1], 2.0)
    assert "_mgar_folded_in" not in conv.state_dict() and len(conv.state_dict()) == 1


# ---- the routing predicate ------------------------------------------------------------------------------------------------------
def _rows(c_in=32, dtype=torch.float32, is_cuda=True, requires_grad=False, ndim=2):
    """what eval_fuse_plan reads of a tensor: nothing but attributes"""
    return types.SimpleNamespace(dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad, ndim=ndim, shape=(100, c_in)[:ndim] if ndim <= 2
                                 else (1, c_in, 100))


def _module(mlps=((32, 32, 32),), pool="max_pool"):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    n = len(mlps)
    return V.NeighborVoxelSAModuleMSG(query_ranges=[[4, 4, 4]] * n, radii=[0.8] * n, nsamples=[16] * n, mlps=[list(m) for m in mlps],
                                      pool_method=pool).eval()


def test_eval_fuse_plan(monkeypatch):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
    xyz = _rows(3)
    plan = lambda mod, feats=None, k=0: V.eval_fuse_plan(mod, k, feats or _rows(mod.mlps_in[k][0].in_channels), xyz)   # noqa: E731
    with torch.no_grad():
        mod = _module(((64, 32, 32), (64, 16, 7)))
        got = plan(mod)
        assert got is not None and got[0] is mod.mlps_in[0][0] and got[1] is mod.mlps_in[0][1] and got[2] is mod.mlps_pos[0][0]
        assert got[3] is mod.mlps_pos[0][1] and got[4] is mod.mlps_out[0][0] and got[5] is mod.mlps_out[0][1] and got[6] is True
        assert plan(mod, k=1)[4].out_channels == 7
        assert plan(mod, _rows(64, torch.bfloat16)) is not None
        assert plan(mod, _rows(64, torch.float16)) is None and plan(mod, _rows(64, torch.float64)) is None
        assert plan(mod, _rows(64, is_cuda=False)) is None                                  # host tensors: the reference's op chain
        assert V.eval_fuse_plan(mod, 0, _rows(64), _rows(3, is_cuda=False)) is None
        assert plan(mod, _rows(64, ndim=3)) is None and plan(mod, _rows(48)) is None        # not (N, C_in) rows
        mod.train()                                                                         # training BatchNorms: batch statistics
        assert plan(mod) is None
        mod.eval()
        for bn in (mod.mlps_in[0][1], mod.mlps_pos[0][1], mod.mlps_out[0][1]):              # each BatchNorm's own flag counts
            bn.train()
            assert plan(mod) is None and plan(mod, k=1) is not None
            bn.eval()
            assert plan(mod) is not None
        for which in ("mlps_in", "mlps_pos", "mlps_out"):                                   # a missing running statistic
            bare = _module()
            old = getattr(bare, which)[0][1]
            getattr(bare, which)[0][1] = type(old)(old.num_features, track_running_stats=False).eval()
            assert plan(bare) is None, which
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", False)                                 # the switch
        assert plan(mod) is None
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
        mod.fused = False
        assert plan(mod) is None
        mod.fused = True
        assert plan(_module(pool="avg_pool")) is None
        assert plan(_module(((64, 48, 32),))) is None and plan(_module(((64, 32, 48),))) is None     # C = 48, Co = 48
        assert plan(_module(((64, 32, 32),))) is not None
        no_relu = _module()
        no_relu.mlps_out[0] = type(no_relu.mlps_out[0])(*list(no_relu.mlps_out[0])[:2])
        assert plan(no_relu)[6] is False
        extra = _module()
        extra.mlps_in[0] = type(extra.mlps_in[0])(*(list(extra.mlps_in[0]) + [nn.ReLU()]))  # not [conv, BN]
        assert plan(extra) is None
        biased = _module()
        biased.mlps_pos[0][0] = nn.Conv2d(3, 32, 1, bias=True)                              # a bias goes into the shift
        assert plan(biased) is not None
        wide = _module()
        wide.mlps_in[0][0] = nn.Conv1d(32, 32, 3, padding=1, bias=False)                    # not point-wise
        assert plan(wide) is None
        for pick in (lambda m: m.mlps_in[0][0], lambda m: m.mlps_pos[0][1], lambda m: m.mlps_out[0][2], lambda m: m.mlps_out[0],
                     lambda m: m.mlps_in[0]):
            hooked = _module()
            pick(hooked).register_forward_hook(lambda m, a, o: None)                        # a hook must see its module run
            assert plan(hooked) is None
        pre = _module()
        pre.mlps_pos[0].register_forward_pre_hook(lambda m, a: None)
        assert plan(pre) is None
    # a gradient: grad mode on and a parameter (or the features) requiring one
    mod = _module()
    assert plan(mod) is None
    for p in mod.parameters():
        p.requires_grad_(False)
    assert plan(mod) is not None
    assert plan(mod, _rows(32, requires_grad=True)) is None
    mod.mlps_out[0][1].bias.requires_grad_(True)
    assert plan(mod) is None
    with torch.no_grad():
        assert plan(mod, _rows(32, requires_grad=True)) is not None


def test_head_would_fuse_the_shipped_layers(monkeypatch):
    """Every scale of the three pool layers at the mil3 spec is fusable in eval mode, none in train mode."""
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
    with torch.no_grad():
        for spec in ([[32, 32, 32]], [[64, 32, 32]]):
            mod = _module(spec)
            assert V.eval_fuse_plan(mod, 0, _rows(spec[0][0]), _rows(3)) is not None
            assert V.eval_fuse_plan(mod.train(), 0, _rows(spec[0][0]), _rows(3)) is None


def test_host_route_reaches_the_new_entry_with_leading_dimensions(monkeypatch):
    """The shim hands the kernel a column slice of a wider buffer through ld_out and refuses rows it cannot describe.  No device:
    L.call records its arguments."""
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as P
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append((name, a)) or 0)
    monkeypatch.setattr(L, "dev_ptr", lambda t, dtype=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(L, "stream_of", lambda t: None)
    monkeypatch.setattr(P, "_rows_ptr", lambda t, dtype, what, real=P._rows_ptr: real(_Dev(t), dtype, what))
    for dt, name in ((torch.float32, FP32), (torch.bfloat16, BF16)):
        del calls[:]
        feats = torch.zeros((50, 12), dtype=dt)
        buf = torch.zeros((9, 96), dtype=dt)
        out = buf[:, 32:39]
        v = lambda *s: torch.zeros(s)                                                        # noqa: E731
        P.voxel_roi_pool_eval_fwd(9, 4, 10, 7, v(50, 3), v(9, 3), feats, torch.zeros((9, 4), dtype=torch.int32), v(10, 3), v(10), v(10),
                                  v(7, 10), v(7), v(7), True, out)
        (got, a), = calls
        assert got == name and a[:4] == (9, 4, 10, 7) and a[7] == 12 and a[15] == 1 and a[17] == 96
        assert a[6] == feats.data_ptr() and a[16] == buf.data_ptr() + 32 * buf.element_size()
        with pytest.raises(L.MgarError):
            P.voxel_roi_pool_eval_fwd(9, 4, 10, 7, v(50, 3), v(9, 3), feats, torch.zeros((9, 4), dtype=torch.int32), v(10, 3), v(10), v(10),
                                      v(7, 10), v(7), v(7), True, buf.t()[:9, :7])
        with pytest.raises(L.MgarError):
            P.voxel_roi_pool_eval_fwd(9, 4, 10, 7, v(50, 3), v(9, 3), feats, torch.zeros((9, 4), dtype=torch.int32), v(10, 3), v(10), v(10),
                                      v(7, 10), v(7), v(7), True, buf[:, :8])


class _Dev:
    """a host tensor that answers is_cuda = True (host-side stand-in for device rows)"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)
