"""mgar_pointwise_mfma_bf16_fwd (csrc/pointwise_bf16.hip) without a device: the ABI surface, the bound of
tests/pointwise_bf16_cases.py pinned as satisfiable (fp32 restatements of the kernel in two summation orders lie inside it) and as
sharp (wrong restatements leave it), and the host decision function on attribute stand-ins."""
import ctypes
import os
import re
import types

import pytest
import torch

import pointwise_bf16_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SYMBOL = "mgar_pointwise_mfma_bf16_fwd"


def test_header_declares_the_symbol():
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    assert re.search(r"^int %s\(const void \*x, int B, int Cin, int P, const float \*w, int w_row_stride, int w_col_stride,\s*"
                     r"int Cout, const float \*in_mean, const float \*in_invstd, const float \*in_gamma,\s*"
                     r"const float \*in_beta, int in_relu, void \*y, void \*stream\);" % SYMBOL, text, flags=re.M)
    assert re.search(r"^#define MGAR_ABI_VERSION 22\b", text, flags=re.M)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert SYMBOL in integration


def test_library_exports_the_symbol_and_abi_22():
    from multimodal_gar_amd import _lib, op_timer
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, SYMBOL)
    assert cdll.mgar_abi_version() == 22 and _lib.ABI_VERSION == 22
    I, P = ctypes.c_int, ctypes.c_void_p
    fn = _lib._fns[SYMBOL]
    assert fn.restype is I and list(fn.argtypes) == [P, I, I, I, P, I, I, I, P, P, P, P, I, P, P]
    # called by name: no payload twin, and the widening entry point keeps its twin
    assert "mgar_pointwise_mfma" not in _lib.BF16_TWINS and "mgar_pointwise_conv_fwd" in _lib.BF16_TWINS
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "pointwise_bf16_kernel" in names and "pointwise_fwd_kernel" in names and len(set(names)) == len(names)
    assert op_timer.KERNEL_SOURCES.get("pointwise_bf16_kernel") == "pointwise_bf16.hip"


def test_case_list_is_the_issues():
    shapes = [c[:4] for c in PC.CASES]
    assert shapes == [(1, 1, 1, 4), (1, 16, 32, 128), (3, 35, 20, 4096), (2, 17, 33, 132), (1, 64, 64, 124), (2, 256, 64, 260),
                      (3, 32, 64, 644), (2, 48, 40, 512)]
    assert [c[4] for c in PC.CASES] == [False] * 7 + [True]
    assert PC.VARIANTS == ("identity", "bn_relu", "bn_noaffine")
    ops = PC.operands(PC.CASES[7], "bn_relu")
    assert ops["strides"] == (1, 40) and ops["w_store"].shape == (48, 40) and torch.equal(ops["w_store"].t(), ops["w"])
    assert ops["x"].dtype == BF and float(ops["invstd"].min()) >= 0.5 and ops["relu"] == 1
    none = PC.operands(PC.CASES[1], "bn_noaffine")
    assert none["gamma"] is None and none["beta"] is None and none["mean"] is not None and none["relu"] == 0
    assert PC.operands(PC.CASES[1], "identity")["mean"] is None


def _kernel_order(a, wt):
    """fp32 accumulation over 16-channel k-steps ascending (the kernel's outer order), one rounding to bf16."""
    acc = torch.zeros((a.shape[0], wt.shape[0], a.shape[2]), dtype=torch.float32)
    for k0 in range(0, a.shape[1], 16):
        acc = acc + torch.einsum("oi,bip->bop", wt[:, k0:k0 + 16], a[:, k0:k0 + 16])
    return acc.to(BF)


def _reversed_order(a, wt):
    """fp32 accumulation one channel at a time, last channel first."""
    acc = torch.zeros((a.shape[0], wt.shape[0], a.shape[2]), dtype=torch.float32)
    for i in reversed(range(a.shape[1])):
        acc = acc + wt[None, :, i, None] * a[:, None, i, :]
    return acc.to(BF)


@pytest.mark.parametrize("variant", PC.VARIANTS)
@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_fp32_restatements_lie_inside_the_bound(case, variant):
    a, wt = PC.rounded_operands(PC.operands(case, variant))
    ref, bound = PC.expected(case, variant)
    for order in (_kernel_order, _reversed_order):
        used = PC.share_of_bound(order(a, wt).float(), ref, bound)
        assert used <= 1.0, (order.__name__, used)


def _leaves(y, case, variant):
    ref, bound = PC.expected(case, variant)
    return PC.share_of_bound(y.float(), ref, bound) > 1.0


def test_wrong_restatements_leave_the_bound():
    case, sq, odd = PC.CASES[2], PC.CASES[4], PC.CASES[3]            # (3, 35, 20, 4096), (1, 64, 64, 124), (2, 17, 33, 132)
    ops = PC.operands(case, "bn_relu")
    a, wt = PC.rounded_operands(ops)
    assert not _leaves(_kernel_order(a, wt), case, "bn_relu")
    # ReLU dropped
    a_norelu = PC.activated(ops["x"], ops["mean"], ops["invstd"], ops["gamma"], ops["beta"], 0).to(BF).float()
    assert _leaves(_kernel_order(a_norelu, wt), case, "bn_relu")
    # channel index off by one (the prologue constants and the weight column of the neighbouring channel)
    assert _leaves(_kernel_order(torch.roll(a, 1, dims=1), wt), case, "bn_relu")
    # W transposed (a square layer: the shapes still fit)
    for variant in PC.VARIANTS:
        a_s, wt_s = PC.rounded_operands(PC.operands(sq, variant))
        assert _leaves(_kernel_order(a_s, wt_s.t().contiguous()), sq, variant)
    # a padding channel left non-zero: the k-step is padded from 17 to 32 channels; the activation of the padding lanes is
    # act(0) of channel 0's constants instead of zero and the weight read runs on into the next row
    ops_o = PC.operands(odd, "bn_relu")
    a_o, wt_o = PC.rounded_operands(ops_o)
    cin, cout = a_o.shape[1], wt_o.shape[0]
    pad = 32 - cin
    act0 = PC.activated(torch.zeros(1, 1, 1, dtype=BF), ops_o["mean"][:1], ops_o["invstd"][:1], ops_o["gamma"][:1], ops_o["beta"][:1], 1)
    assert float(act0) != 0.0
    a_pad = torch.cat([a_o, act0.to(BF).float().expand(a_o.shape[0], pad, a_o.shape[2])], 1)
    flat = torch.cat([wt_o.reshape(-1), wt_o.reshape(-1)])
    w_pad = torch.stack([flat[o * cin:o * cin + 32] for o in range(cout)])
    assert torch.equal(w_pad[:, :cin], wt_o)
    assert _leaves(_kernel_order(a_pad, w_pad), odd, "bn_relu")
    # output rounded twice, through fp16: values just below an odd bf16 tie go the wrong way
    acc = torch.einsum("oi,bip->bop", wt, a)
    assert not _leaves(acc.to(BF), case, "bn_relu")
    assert _leaves(acc.half().to(BF), case, "bn_relu")


def _x(dtype=BF, shape=(2, 16, 1024, 32), cuda=True):
    return types.SimpleNamespace(dtype=dtype, is_cuda=cuda, shape=shape)


def _bn(training=True):
    return types.SimpleNamespace(training=training)


def test_decision_function(monkeypatch):
    """mlp_bf16_mfma_plan on stand-ins that carry attributes only: true for the intersection of the conditions, false when any
    one of them fails."""
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", True)
    plan = bn_ops.mlp_bf16_mfma_plan
    assert plan(_x(), 32, False, _bn()) is True
    assert plan(_x(), 32, False, None) is True                                      # no prologue (plain_conv)
    assert plan(_x(shape=(1, 64, 65536)), 64, False, _bn()) is True                 # the widest layer, exactly 65 536 columns
    assert plan(_x(shape=(4, 1, 128, 128)), 1, False, _bn()) is True
    assert not plan(_x(dtype=torch.float32), 32, False, _bn())                      # fp32 payload
    assert not plan(_x(dtype=torch.float16), 32, False, _bn())
    assert not plan(_x(cuda=False), 32, False, _bn())                               # not on the device
    assert not plan(_x(), 32, True, _bn())                                          # a gradient is required
    assert not plan(_x(), 32, False, _bn(training=False))                           # eval-mode BatchNorm: the inference route
    assert not plan(_x(shape=(2, 65, 1024, 32)), 32, False, _bn())                  # C = 65
    assert not plan(_x(), 65, False, _bn())                                         # Cout = 65
    assert not plan(_x(shape=(2, 16, 32770)), 32, False, _bn())                     # P % 4 != 0
    assert not plan(_x(shape=(2, 16, 1024, 31)), 32, False, _bn())                  # fewer than 65 536 columns
    assert not plan(_x(shape=(1, 16, 65532)), 32, False, _bn())
    assert not plan(_x(shape=(2, 16)), 32, False, _bn())
    # plain_conv's own gates: 32 / 32
    assert plan(_x(shape=(2, 32, 1024, 32)), 32, False, None, bn_ops.PLAIN_CONV_MAX_IN, bn_ops.PLAIN_CONV_MAX_OUT) is True
    assert not plan(_x(shape=(2, 33, 1024, 32)), 32, False, None, bn_ops.PLAIN_CONV_MAX_IN, bn_ops.PLAIN_CONV_MAX_OUT)
    assert not plan(_x(), 33, False, None, bn_ops.PLAIN_CONV_MAX_IN, bn_ops.PLAIN_CONV_MAX_OUT)
    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", False)                             # switch off
    assert not plan(_x(), 32, False, _bn())
    assert not plan(_x(), 32, False, None)

