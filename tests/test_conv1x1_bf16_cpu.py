"""mgar_conv1x1_bf16_fwd / mgar_conv1x1_bf16_fwd_affine (csrc/pointwise_wide_bf16.hip) without a device: the ABI surface, the bounds of
tests/conv1x1_bf16_cases.py pinned as satisfiable (fp32 restatements of the kernel in two k-step orders lie inside them) and as
sharp (wrong restatements leave them), Unit3D's routing predicates on attribute stand-ins, and the weight cache."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv1x1_bf16_cases as K
import sparse_conv_affine_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
PLAIN, AFFINE = "mgar_conv1x1_bf16_fwd", "mgar_conv1x1_bf16_fwd_affine"


# ---- the ABI surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    assert re.search(r"^int %s\(const void \*x, int N, int Cin, int P, const float \*w, int Cout,\s*"
                     r"void \*y, long long y_batch_stride, void \*stream\);" % PLAIN, text, flags=re.M)
    assert re.search(r"^int %s\(const void \*x, int N, int Cin, int P, const float \*w, int Cout,\s*"
                     r"const float \*scale, const float \*shift, int relu,\s*"
                     r"void \*y, long long y_batch_stride, void \*stream\);" % AFFINE, text, flags=re.M)
    assert re.search(r"^#define MGAR_ABI_VERSION 22\b", text, flags=re.M)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert PLAIN in integration and AFFINE in integration


def test_library_exports_the_symbols_and_abi_22():
    from multimodal_gar_amd import _lib, op_timer
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, PLAIN) and hasattr(cdll, AFFINE)
    assert cdll.mgar_abi_version() == 22 and _lib.ABI_VERSION == 22
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    assert _lib._fns[PLAIN].restype is I and list(_lib._fns[PLAIN].argtypes) == [P, I, I, I, P, I, P, LL, P]
    assert _lib._fns[AFFINE].restype is I and list(_lib._fns[AFFINE].argtypes) == [P, I, I, I, P, I, P, P, I, P, LL, P]
    assert "mgar_conv1x1" not in _lib.BF16_TWINS                                    # called by name: no payload twin
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "conv1x1_bf16_kernel" in names and names[-1] != "conv1x1_bf16_kernel" and len(set(names)) == len(names)
    assert names[-1] == "voxel_roi_pool_eval"
    assert op_timer.KERNEL_SOURCES.get("conv1x1_bf16_kernel") == "pointwise_wide_bf16.hip"
    assert os.path.exists(os.path.join(ROOT, "multimodal_gar_amd", "csrc", "pointwise_wide_bf16.hip"))


def test_case_list_is_the_issues():
    assert K.CASES == ((1, 8, 8, 4), (1, 64, 64, 132), (1, 40, 24, 516), (2, 192, 96, 96), (2, 480, 16, 180), (3, 528, 256, 260),
                       (2, 832, 384, 8))
    for case in K.CASES:
        x, w = K.operands(case)
        assert x.shape == (case[0], case[1], case[3]) and w.shape == (case[2], case[1])
        assert torch.equal(x.to(BF).float(), x) and torch.equal(w.to(BF).float(), w) and float(x.min()) >= 0.0
        e = K.expected(case)
        assert e["scale"][0] < 0 and e["scale"][1] == 0 and e["scale"][2] == 1000.0


# ---- restatements of the kernel -------------------------------------------------------------------------------------------------
def _acc(x, w, descending=False, steps=None):
    """fp32 accumulation over 16-channel k-steps (ascending: the kernel's outer order), no final rounding -> float32 tensor"""
    starts = list(range(0, x.shape[1], 16))[:steps]
    acc = torch.zeros((x.shape[0], w.shape[0], x.shape[2]), dtype=torch.float32)
    for k0 in (reversed(starts) if descending else starts):
        acc = acc + torch.einsum("oi,bip->bop", w[:, k0:k0 + 16], x[:, k0:k0 + 16])
    return acc


def _affine(acc, scale, shift, relu):
    return A.emulate_epilogue(acc.numpy(), K.per_channel(scale), K.per_channel(shift), relu, True)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_fp32_restatements_lie_inside_the_bounds(case):
    e = K.expected(case)
    for descending in (False, True):
        acc = _acc(e["x"], e["w"], descending)
        assert K.plain_share(acc.to(BF).float(), case) <= 1.0, descending
        for relu in (0, 1):
            assert K.affine_share(_affine(acc, e["scale"], e["shift"], relu), case, relu) <= 1.0, (descending, relu)


def _leaves_somewhere(make_acc=None, scale_of=None, relu_applied=None):
    """-> (plain leaves on a case, affine leaves on a case) for a wrong restatement"""
    plain = affine = False
    for case in K.CASES:
        e = K.expected(case)
        acc = make_acc(case, e) if make_acc else _acc(e["x"], e["w"])
        plain = plain or K.plain_share(acc.to(BF).float(), case) > 1.0
        scale, shift = scale_of(e) if scale_of else (e["scale"], e["shift"])
        for relu in (0, 1):
            got = _affine(acc, scale, shift, relu if relu_applied is None else relu_applied)
            affine = affine or K.affine_share(got, case, relu) > 1.0
    return plain, affine


def test_wrong_restatements_leave_the_bounds():
    # the last k-step dropped
    assert _leaves_somewhere(lambda case, e: _acc(e["x"], e["w"], steps=(case[1] + 15) // 16 - 1)) == (True, True)
    # the weight left unrounded
    assert _leaves_somewhere(lambda case, e: _acc(e["x"], K.unrounded_weight(case))) == (True, True)
    # the neighbouring channel's scale / shift
    assert _leaves_somewhere(scale_of=lambda e: (np.roll(e["scale"], 1), np.roll(e["shift"], 1))) == (False, True)
    # the ReLU missing
    assert _leaves_somewhere(relu_applied=0) == (False, True)


# ---- the routing predicates -----------------------------------------------------------------------------------------------------
def _like(shape, dtype=BF, is_cuda=True, requires_grad=False, contiguous=True):
    """what the predicates read of the input: nothing but attributes"""
    return types.SimpleNamespace(shape=torch.Size(shape), dtype=dtype, is_cuda=is_cuda, requires_grad=requires_grad,
                                 dim=lambda: len(shape), is_contiguous=lambda: contiguous)


def _switches(monkeypatch, gemm=True, k1=True, fold=True):
    from multimodal_gar_amd.model.backbone import Unit3D
    monkeypatch.setattr(Unit3D, "gemm_1x1", gemm)
    monkeypatch.setattr(Unit3D, "k1_bf16", k1)
    monkeypatch.setattr(Unit3D, "fold_bn_eval", fold)
    return Unit3D


def test_k1_bf16_route_conditions(monkeypatch):
    Unit3D = _switches(monkeypatch)
    u = Unit3D(48, 40, [1, 1, 1]).eval()
    x = _like((2, 48, 3, 4, 6))
    with torch.no_grad():
        assert u._k1_bf16_route(x) is True
        u.conv3d.weight.data = u.conv3d.weight.data.to(BF)                              # a bf16 weight, as ForwardStep converts it
        assert u._k1_bf16_route(x) is True
        u.conv3d.weight.data = u.conv3d.weight.data.half()
        assert u._k1_bf16_route(x) is False
        u.conv3d.weight.data = u.conv3d.weight.data.float()
        assert u._k1_bf16_route(_like((2, 48, 3, 4, 6), dtype=torch.float32)) is False   # fp32 payload
        assert u._k1_bf16_route(_like((2, 48, 3, 4, 6), dtype=torch.float16)) is False
        assert u._k1_bf16_route(_like((2, 48, 3, 4, 6), is_cuda=False)) is False         # host tensor
        assert u._k1_bf16_route(_like((2, 48, 3, 4, 6), contiguous=False)) is False      # channels-last activations
        assert u._k1_bf16_route(_like((2, 48, 3, 5, 7))) is False                        # P % 4 != 0
        assert u._k1_bf16_route(_like((2, 48, 1, 2, 2))) is True
        assert u._k1_bf16_route(_like((2, 48, 12, 6))) is False                          # not 5-D
        _switches(monkeypatch, gemm=False)
        assert u._k1_bf16_route(x) is False                                             # inside gemm_1x1
        _switches(monkeypatch, k1=False)
        assert u._k1_bf16_route(x) is False                                             # the switch
        _switches(monkeypatch)
        assert Unit3D(48, 40, [3, 3, 3]).eval()._k1_bf16_route(x) is False
        assert Unit3D(48, 40, [1, 1, 1], stride=(1, 2, 2)).eval()._k1_bf16_route(x) is False
        assert Unit3D(48, 40, [1, 1, 1], use_bias=True).eval()._k1_bf16_route(x) is False
        grouped = Unit3D(48, 40, [1, 1, 1]).eval()
        grouped.conv3d = nn.Conv3d(48, 40, 1, groups=2, bias=False)
        assert grouped._k1_bf16_route(x) is False
        assert Unit3D(1024, 512, [1, 1, 1]).eval()._k1_bf16_route(_like((1, 1024, 1, 2, 2))) is True
        assert Unit3D(1025, 8, [1, 1, 1]).eval()._k1_bf16_route(_like((1, 1025, 1, 2, 2))) is False
        assert Unit3D(8, 513, [1, 1, 1]).eval()._k1_bf16_route(_like((1, 8, 1, 2, 2))) is False
    # a gradient: grad mode on and the weight (or the input) requiring one
    assert u._k1_bf16_route(x) is False
    u.conv3d.weight.requires_grad_(False)
    assert u._k1_bf16_route(x) is True
    assert u._k1_bf16_route(_like((2, 48, 3, 4, 6), requires_grad=True)) is False


def test_eval_fold_plan_1x1_conditions(monkeypatch):
    Unit3D = _switches(monkeypatch)
    u = Unit3D(48, 40, [1, 1, 1]).eval()
    x = _like((2, 48, 3, 4, 6))
    with torch.no_grad():
        assert u.eval_fold_plan_1x1(x) == "k1_bf16" and u.eval_fold_plan(x) is None       # eval_fold_plan never folds a 1x1x1 unit
        assert u.eval_fold_plan(_like((2, 48, 3, 4, 6), dtype=torch.float32)) is None
        u.train()
        assert u.eval_fold_plan_1x1(x) is None and u._k1_bf16_route(x) is True            # train mode: the plain kernel + statistics
        u.eval()
        u.bn.train()
        assert u.eval_fold_plan_1x1(x) is None
        u.bn.eval()
        _switches(monkeypatch, fold=False)
        assert u.eval_fold_plan_1x1(x) is None and u._k1_bf16_route(x) is True            # the plain kernel + bn_act
        _switches(monkeypatch, k1=False)
        assert u.eval_fold_plan_1x1(x) is None
        _switches(monkeypatch, gemm=False)
        assert u.eval_fold_plan_1x1(x) is None
        _switches(monkeypatch)
        assert u.eval_fold_plan_1x1(_like((2, 48, 3, 4, 6), dtype=torch.float32)) is None  # fp32 input
        assert u.eval_fold_plan_1x1(_like((2, 48, 3, 5, 7))) is None                       # P % 4 != 0
        assert u.eval_fold_plan_1x1(_like((2, 48, 3, 4, 6), is_cuda=False)) is None
        assert u.eval_fold_plan_1x1(_like((2, 48, 3, 4, 6), contiguous=False)) is None
        u.emit_channels_last = True
        assert u.eval_fold_plan_1x1(x) is None
        u.emit_channels_last = False
        nostat = Unit3D(48, 40, [1, 1, 1]).eval()
        nostat.bn = nn.BatchNorm3d(40, eps=1e-3, track_running_stats=False).eval()
        assert nostat.eval_fold_plan_1x1(x) is None
        assert Unit3D(48, 40, [1, 1, 1], activation_fn=torch.tanh).eval().eval_fold_plan_1x1(x) is None
        assert Unit3D(48, 40, [1, 1, 1], activation_fn=None).eval().eval_fold_plan_1x1(x) == "k1_bf16"
        assert Unit3D(48, 40, [1, 1, 1], use_batch_norm=False).eval().eval_fold_plan_1x1(x) is None
        assert Unit3D(48, 40, [3, 3, 3]).eval().eval_fold_plan_1x1(x) is None               # eval_fold_plan's unit
        assert Unit3D(48, 40, [3, 3, 3]).eval().eval_fold_plan(x) == "k3_bf16"
    # a gradient: the convolution weight, the BatchNorm's affine parameters, the input
    assert u.eval_fold_plan_1x1(x) is None
    u.conv3d.weight.requires_grad_(False)
    assert u.eval_fold_plan_1x1(x) is None and u._k1_bf16_route(x) is True
    u.bn.weight.requires_grad_(False)
    u.bn.bias.requires_grad_(False)
    assert u.eval_fold_plan_1x1(x) == "k1_bf16"
    assert u.eval_fold_plan_1x1(_like((2, 48, 3, 4, 6), requires_grad=True)) is None


def test_eval_fold_plan_still_none_for_the_trunks_1x1x1_units(monkeypatch):
    Unit3D = _switches(monkeypatch)
    from multimodal_gar_amd.model.backbone import InceptionI3d
    net = InceptionI3d(final_endpoint="Mixed_4f")
    net.build()
    net.eval()
    ones = [m for m in net.modules() if isinstance(m, Unit3D) and m._kernel_shape == (1, 1, 1)]
    assert len(ones) == 29
    with torch.no_grad():
        for u in ones:
            for dtype in (torch.float32, BF):
                assert u.eval_fold_plan(_like((1, u.conv3d.in_channels, 4, 12, 16), dtype=dtype)) is None
            assert u.eval_fold_plan_1x1(_like((1, u.conv3d.in_channels, 4, 12, 16))) == "k1_bf16"
            assert u.eval_fold_plan_1x1(_like((1, u.conv3d.in_channels, 4, 12, 16), dtype=torch.float32)) is None


def test_weight_cache_recomputes_after_an_update():
    from multimodal_gar_amd.model.backbone import Unit3D
    torch.manual_seed(3)
    u = Unit3D(12, 20, [1, 1, 1]).eval()
    u.conv3d.weight.data = u.conv3d.weight.data.to(BF)
    w0 = u._k1_weight()
    assert w0.dtype == torch.float32 and w0.shape == (20, 12) and w0.is_contiguous() and not w0.requires_grad
    assert torch.equal(w0, u.conv3d.weight.detach().float().view(20, 12))                # widened exactly
    assert u._k1_weight() is w0                                                        # nothing computed
    with torch.no_grad():
        u.conv3d.weight.mul_(2.0)                                                      # an in-place update
    w1 = u._k1_weight()
    assert w1 is not w0 and torch.equal(w1, 2.0 * w0) and u._k1_weight() is w1
    u.conv3d.weight.data = torch.randn(20, 12, 1, 1, 1)                                 # .data replaced (an fp32 master weight)
    w2 = u._k1_weight()
    assert w2 is not w1 and torch.equal(w2, u.conv3d.weight.detach().view(20, 12)) and u._k1_weight() is w2
    assert "_mgar_k1_weight" not in u.state_dict() and len(u.state_dict()) == 6
