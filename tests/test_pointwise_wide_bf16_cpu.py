"""mgar_pointwise_wide_bf16_fwd / mgar_pointwise_wide_maxpool_bf16_fwd (csrc/pointwise_wide_bf16.hip) without a device: the ABI
surface, the bounds of tests/pointwise_wide_bf16_cases.py pinned as satisfiable (an fp32 restatement of the contract lies inside
them) and as sharp (restatements that forget a rounding, a ReLU or half a group leave them), and the host decision function
bn_ops.mlp_bf16_wide_plan on attribute stand-ins."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import pointwise_bf16_cases as PC
import pointwise_wide_bf16_cases as WC
import sparse_conv_affine_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
FWD, POOL = "mgar_pointwise_wide_bf16_fwd", "mgar_pointwise_wide_maxpool_bf16_fwd"


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------
def test_header_declares_both_symbols():
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    assert re.search(r"^int %s\(const void \*x, int B, int Cin, int P, const float \*w, int w_ld, int Cout,\s*"
                     r"const float \*in_mean, const float \*in_invstd, const float \*in_gamma, const float \*in_beta,\s*"
                     r"int in_relu, const float \*out_scale, const float \*out_shift, int out_relu, void \*y,\s*"
                     r"long long y_batch_stride, void \*stream\);" % FWD, text, flags=re.M)
    assert re.search(r"^int %s\(const void \*x, int B, int Cin, int M, int ns, const float \*w, int w_ld, int Cout,\s*"
                     r"const float \*in_mean, const float \*in_invstd, const float \*in_gamma,\s*"
                     r"const float \*in_beta, int in_relu, const float \*out_scale, const float \*out_shift,\s*"
                     r"int out_relu, void \*y, void \*stream\);" % POOL, text, flags=re.M)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert FWD in integration and POOL in integration


def test_library_exports_both_symbols_and_the_timer_row():
    from multimodal_gar_amd import _lib, op_timer
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, FWD) and hasattr(cdll, POOL)
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    fn = _lib._fns[FWD]
    assert fn.restype is I and list(fn.argtypes) == [P, I, I, I, P, I, I, P, P, P, P, I, P, P, I, P, LL, P]
    fn = _lib._fns[POOL]
    assert fn.restype is I and list(fn.argtypes) == [P, I, I, I, I, P, I, I, P, P, P, P, I, P, P, I, P, P]
    assert not any(n.startswith("mgar_pointwise_wide") for n in _lib.BF16_TWINS)       # called by name: no payload twins
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "pointwise_wide_bf16_kernel" in names and "pointwise_bf16_kernel" in names and "conv1x1_bf16_kernel" in names
    assert len(set(names)) == len(names)
    assert op_timer.KERNEL_SOURCES.get("pointwise_wide_bf16_kernel") == "pointwise_wide_bf16.hip"
    assert os.path.exists(os.path.join(ROOT, "multimodal_gar_amd", "csrc", "pointwise_wide_bf16.hip"))


def test_case_list_is_the_issues():
    assert [c[:4] for c in WC.CASES] == [(1, 1, 1, 4), (2, 17, 65, 132), (1, 99, 64, 256), (2, 128, 33, 516), (1, 259, 128, 128),
                                         (3, 196, 256, 644), (2, 1024, 512, 260), (1, 384, 512, 8), (2, 61, 96, 512)]
    assert [c[4] for c in WC.CASES] == [None] * 8 + [(160, 3)]
    assert [pc[0] for pc in WC.POOLED] == [(1, 64, 128, 8, 4), (2, 196, 256, 33, 16), (3, 128, 65, 100, 32), (2, 17, 96, 7, 64),
                                           (1, 256, 512, 5, 128)]
    assert {pc[1] for pc in WC.POOLED} == set(WC.PROLOGUES) and {pc[2] for pc in WC.POOLED} == {0, 1}
    assert WC.PROLOGUES == ("identity", "bn_relu", "bn_noaffine") and WC.STORES == ("plain", "affine_relu", "affine")
    ops = WC.operands(WC.CASES[8], "bn_relu")
    assert ops["w_full"].shape == (96, 160) and ops["w_ld"] == 160 and ops["w_off"] == 3
    assert torch.equal(ops["w"], ops["w_full"][:, 3:64]) and ops["x"].dtype == BF and ops["relu"] == 1
    assert (ops["w_off"] * 4) % 16 != 0                                                 # the slice's pointer is misaligned
    # the affine vectors: a negative, an exact zero and a large channel; shifts of both signs
    e = WC.expected(WC.CASES[5], "identity")
    assert e["scale"][0] < 0 and e["scale"][1] == 0 and e["scale"][2] == 1000 and (e["shift"] > 0).any() and (e["shift"] < 0).any()
    # the pooled shift zeroes whole groups behind out_relu, and not all of them
    for pc in WC.POOLED:
        p = WC.pooled_expected(pc)
        if pc[2]:
            even = p["ref"][:, 0::2]
            assert (even == 0).any() and (even > 0).any(), WC.pooled_id(pc)


# ---- the bounds are satisfiable and sharp -----------------------------------------------------------------------------------------
def _acc(a, wt):
    """the fp32 accumulator: 16-channel k-steps ascending (the kernel's outer order) -> (B, Cout, P) float32 tensor"""
    acc = torch.zeros((a.shape[0], wt.shape[0], a.shape[2]), dtype=torch.float32)
    for k0 in range(0, a.shape[1], 16):
        acc = acc + torch.einsum("oi,bip->bop", wt[:, k0:k0 + 16], a[:, k0:k0 + 16])
    return acc


def _store(acc, scale, shift, relu):
    """the store of the contract on an fp32 accumulator -> float32 numpy holding bf16 values"""
    if scale is None:
        return acc.to(BF).float().numpy()
    return A.emulate_epilogue(acc.numpy(), WC.per_channel(scale), WC.per_channel(shift), relu, True)


def _pooled(acc, scale, shift, relu, ns):
    """fmaf, ReLU, max over the group in fp32, ONE rounding -> float32 numpy (B, Cout, M)"""
    v = A.emulate_epilogue(acc.numpy(), WC.per_channel(scale), WC.per_channel(shift), relu, False)
    b, cout, p = v.shape
    return A.B.to_bf16(v.reshape(b, cout, p // ns, ns).max(axis=3))


@pytest.mark.parametrize("prologue", WC.PROLOGUES)
@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_fp32_restatement_lies_inside_the_bounds(case, prologue):
    a, wt = WC.rounded_operands(WC.operands(case, prologue))
    acc = _acc(a, wt)
    for store in WC.STORES:
        scale, shift, relu = WC.store_args(case, prologue, store)
        ref, bound = WC.store_expected(case, prologue, store)
        used = WC.share(_store(acc, scale, shift, relu), ref, bound)
        assert used <= 1.0, (store, used)


@pytest.mark.parametrize("pc", WC.POOLED, ids=WC.pooled_id)
def test_fp32_restatement_of_the_pooled_store_lies_inside_its_bound(pc):
    a, wt = WC.rounded_operands(WC.operands(WC.pooled_as_case(pc), pc[1]))
    e = WC.pooled_expected(pc)
    used = WC.share(_pooled(_acc(a, wt), e["scale"], e["shift"], pc[2], pc[0][4]), e["ref"], e["bound"])
    assert used <= 1.0, used


def test_wrong_restatements_leave_the_bounds():
    case = WC.CASES[5]                                                                  # (3, 196, 256, 644)
    ops = WC.operands(case, "bn_relu")
    a, wt = WC.rounded_operands(ops)
    acc = _acc(a, wt)

    def leaves(y, store, prologue="bn_relu"):
        ref, bound = WC.store_expected(case, prologue, store)
        return WC.share(y, ref, bound) > 1.0
    sc, sh, _ = WC.store_args(case, "bn_relu", "affine_relu")
    assert not leaves(_store(acc, None, None, 0), "plain") and not leaves(_store(acc, sc, sh, 1), "affine_relu")
    assert not leaves(_store(acc, sc, sh, 0), "affine")
    # a forgotten rounding: the activated input left in fp32; the weight left in fp32
    a32 = PC.activated(ops["x"], ops["mean"], ops["invstd"], ops["gamma"], ops["beta"], ops["relu"])
    assert leaves(_store(_acc(a32, wt), None, None, 0), "plain") and leaves(_store(_acc(a32, wt), sc, sh, 1), "affine_relu")
    assert leaves(_store(_acc(a, ops["w"]), None, None, 0), "plain") and leaves(_store(_acc(a, ops["w"]), sc, sh, 0), "affine")
    # a rounding too many: the accumulator rounded to bf16 before the affine store, the result again after it
    assert leaves(_store(acc.to(BF).float(), sc, sh, 1), "affine_relu")
    # the input ReLU forgotten; the output ReLU forgotten; the output ReLU applied where none is asked for
    a_norelu = PC.activated(ops["x"], ops["mean"], ops["invstd"], ops["gamma"], ops["beta"], 0).to(BF).float()
    assert leaves(_store(_acc(a_norelu, wt), None, None, 0), "plain")
    assert leaves(_store(acc, sc, sh, 0), "affine_relu") and leaves(_store(acc, sc, sh, 1), "affine")
    # the affine forgotten, or taken from the neighbouring channel
    assert leaves(_store(acc, None, None, 0), "affine")
    assert leaves(_store(acc, np.roll(sc, 1), np.roll(sh, 1), 1), "affine_relu")
    # the weight slice read from column 0 instead of column 3
    sl = WC.CASES[8]
    ops_s = WC.operands(sl, "identity")
    a_s, _ = WC.rounded_operands(ops_s)
    ref, bound = WC.store_expected(sl, "identity", "plain")
    assert WC.share(_store(_acc(a_s, ops_s["w"].to(BF).float()), None, None, 0), ref, bound) <= 1.0
    assert WC.share(_store(_acc(a_s, ops_s["w_full"][:, :61].to(BF).float()), None, None, 0), ref, bound) > 1.0
    # pooled: half the group; the output ReLU forgotten; rounded before the affine as the unfused route does
    pc = WC.POOLED[1]                                                                   # (2, 196, 256, 33, 16), identity, relu
    ns = pc[0][4]
    a_p, wt_p = WC.rounded_operands(WC.operands(WC.pooled_as_case(pc), pc[1]))
    acc_p = _acc(a_p, wt_p)
    e = WC.pooled_expected(pc)
    assert WC.share(_pooled(acc_p, e["scale"], e["shift"], 1, ns), e["ref"], e["bound"]) <= 1.0
    v = A.emulate_epilogue(acc_p.numpy(), WC.per_channel(e["scale"]), WC.per_channel(e["shift"]), 1, False)
    half = A.B.to_bf16(v.reshape(2, 256, 33, ns)[..., :ns // 2].max(axis=3))
    assert WC.share(half, e["ref"], e["bound"]) > 1.0
    assert WC.share(_pooled(acc_p, e["scale"], e["shift"], 0, ns), e["ref"], e["bound"]) > 1.0
    assert WC.share(_pooled(acc_p.to(BF).float(), e["scale"], e["shift"], 1, ns), e["ref"], e["bound"]) > 1.0


# ---- the host decision function ---------------------------------------------------------------------------------------------------
def _x(dtype=BF, shape=(2, 128, 1024, 32), cuda=True, requires_grad=False):
    return types.SimpleNamespace(dtype=dtype, is_cuda=cuda, shape=shape, requires_grad=requires_grad)


def _conv(cin, cout, bias=False):
    return nn.Conv2d(cin, cout, 1, bias=bias).requires_grad_(False)


def _bn(c, training=True):
    return nn.BatchNorm2d(c).requires_grad_(False).train(training)


def test_decision_function(monkeypatch):
    """mlp_bf16_wide_plan on stand-ins for x that carry attributes only: true for the intersection of the conditions, false when
    any one of them fails."""
    from multimodal_gar_amd import _lib as L, bn_ops
    monkeypatch.setattr(bn_ops, "MLP_BF16_WIDE", True)
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    plan = bn_ops.mlp_bf16_wide_plan
    # the plan's own gates, narrower than the kernel (set by measurement: profiles/README.md): 128 / 128
    assert (bn_ops.WIDE_MAX_IN, bn_ops.WIDE_MAX_OUT) == (1024, 512)
    assert bn_ops.WIDE_PLAN_MAX_IN <= bn_ops.WIDE_MAX_IN and bn_ops.WIDE_PLAN_MAX_OUT <= bn_ops.WIDE_MAX_OUT
    with torch.no_grad():
        for cin, cout, want in ((64, 128, True), (96, 128, True), (128, 128, True), (1, 128, True), (128, 65, True), (65, 8, True),
                                (128, 196, False), (196, 128, False), (128, 256, False), (256, 128, False), (1024, 512, False)):
            assert (bn_ops.WIDE_PLAN_MAX_IN, bn_ops.WIDE_PLAN_MAX_OUT) == (128, 128)
            assert plan(_x(shape=(2, cin, 1024, 32)), _conv(cin, cout)) is want, (cin, cout)
    # everything below with the plan's gates lifted to the kernel's limits
    monkeypatch.setattr(bn_ops, "WIDE_PLAN_MAX_IN", bn_ops.WIDE_MAX_IN)
    monkeypatch.setattr(bn_ops, "WIDE_PLAN_MAX_OUT", bn_ops.WIDE_MAX_OUT)
    with torch.no_grad():
        assert plan(_x(), _conv(128, 256), _bn(128)) is True                            # train-mode hidden step
        assert plan(_x(), _conv(128, 256)) is True                                      # identity prologue
        assert plan(_x(), _conv(128, 256), _bn(128, False)) is True                     # eval-mode hidden step
        assert plan(_x(), _conv(128, 256), _bn(128, False), _bn(256, False), pool=True) is True
        assert plan(_x(), _conv(128, 256), None, _bn(256, False)) is True               # unpooled affine tail
        assert plan(_x(shape=(1, 1024, 65536)), _conv(1024, 512)) is True               # both limits, exactly 65 536 columns
        assert plan(_x(shape=(2, 65, 1024, 32)), _conv(65, 8)) is True                  # wide by Cin alone
        assert plan(_x(shape=(2, 8, 1024, 32)), _conv(8, 65)) is True                   # wide by Cout alone
        assert plan(_x(shape=(2, 128, 32768)), _conv(256, 64), cin=128) is True         # a column slice of the weight
        # max(C, Cout) <= 64: every shape of tests/test_pointwise_bf16_gpu.py and tests/test_mlp_eval_gpu.py stays where it is
        for cin, cout in ((16, 16), (16, 32), (64, 64), (1, 1), (35, 20), (48, 40), (32, 64), (4, 64), (64, 4)):
            assert not plan(_x(shape=(2, cin, 1024, 32)), _conv(cin, cout), _bn(cin))
            assert not plan(_x(shape=(2, cin, 1024, 32)), _conv(cin, cout))
            assert not plan(_x(shape=(2, cin, 1024, 32)), _conv(cin, cout), _bn(cin, False), _bn(cout, False), pool=True)
        import mlp_eval_cases as ME
        for (b, cin, cout, m, ns), pro, _, _ in ME.CASES:
            assert not plan(_x(shape=(b, cin, m, ns)), _conv(cin, cout), None if pro == "id" else _bn(cin, False), _bn(cout, False),
                            pool=True)
        for b, cin, cout, p, _ in PC.CASES:
            assert not plan(_x(shape=(b, cin, p)), _conv(cin, cout)) and not plan(_x(shape=(b, cin, p)), _conv(cin, cout), _bn(cin))
        assert not plan(_x(dtype=torch.float32), _conv(128, 256), _bn(128))             # fp32 payload
        assert not plan(_x(dtype=torch.float16), _conv(128, 256), _bn(128))
        assert not plan(_x(cuda=False), _conv(128, 256), _bn(128))                      # not on the device
        assert not plan(_x(), _conv(128, 256, bias=True), _bn(128))                     # a bias
        assert not plan(_x(), nn.Conv2d(128, 256, 3, bias=False), _bn(128))             # not point-wise
        assert not plan(_x(shape=(1, 1025, 65536)), _conv(1025, 128))                   # Cin 1025
        assert not plan(_x(), _conv(128, 513))                                          # Cout 513
        assert not plan(_x(shape=(2, 128, 32770)), _conv(128, 256))                     # P % 4 != 0
        assert not plan(_x(shape=(2, 128, 1024, 31)), _conv(128, 256))                  # fewer than 65 536 columns
        assert not plan(_x(shape=(2, 128)), _conv(128, 256))
        assert not plan(_x(shape=(2, 96, 1024, 32)), _conv(128, 256))                   # the conv is not x's
        assert not plan(_x(), _conv(128, 256), _bn(64))
        assert not plan(_x(shape=(2, 128, 32768)), _conv(256, 64), cin=64)
        assert not plan(_x(shape=(2, 128, 4096, 24)), _conv(128, 256), _bn(128, False), _bn(256, False), pool=True)   # ns 24
        assert not plan(_x(shape=(2, 128, 32768)), _conv(128, 256), _bn(128, False), _bn(256, False), pool=True)       # not 4-D
        assert not plan(_x(), _conv(128, 256), _bn(128, False), pool=True)              # a pooled store needs its BatchNorm
        assert not plan(_x(), _conv(128, 256), _bn(128), _bn(256, True))                # a train-mode BatchNorm cannot be folded
        norun = nn.BatchNorm2d(128, track_running_stats=False).requires_grad_(False).eval()
        assert not plan(_x(), _conv(128, 256), norun)                                   # eval mode without running statistics
        hooked = _conv(128, 256)
        hooked.register_forward_hook(lambda *a: None)
        assert not plan(_x(), hooked, _bn(128))                                         # a forward hook
        relu = nn.ReLU()
        relu.register_forward_pre_hook(lambda *a: None)
        assert not plan(_x(), _conv(128, 256), _bn(128), others=(relu,))
        assert plan(_x(), _conv(128, 256), _bn(128), others=(nn.ReLU(),)) is True
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", False)                             # the eval forms follow MLP_EVAL_FUSE
        assert not plan(_x(), _conv(128, 256), _bn(128, False))
        assert not plan(_x(), _conv(128, 256), None, _bn(256, False))
        assert plan(_x(), _conv(128, 256), _bn(128)) is True
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    # a required gradient: grad mode on and x, or a parameter of the swallowed layers, wants one
    assert plan(_x(), _conv(128, 256), _bn(128)) is True
    assert not plan(_x(requires_grad=True), _conv(128, 256), _bn(128))
    assert not plan(_x(), nn.Conv2d(128, 256, 1, bias=False), _bn(128))
    assert not plan(_x(), _conv(128, 256), nn.BatchNorm2d(128))
    with torch.no_grad():
        assert plan(_x(requires_grad=True), nn.Conv2d(128, 256, 1, bias=False), nn.BatchNorm2d(128)) is True
        whole = L._fns
        fns = dict(whole)                                                               # a library without the symbol
        del fns[FWD]
        monkeypatch.setattr(L, "_fns", fns)
        assert not plan(_x(), _conv(128, 256), _bn(128))
        assert plan(_x(), _conv(128, 256), _bn(128, False), _bn(256, False), pool=True) is True
        del fns[POOL]
        assert not plan(_x(), _conv(128, 256), _bn(128, False), _bn(256, False), pool=True)
        monkeypatch.setattr(L, "_fns", whole)
        assert plan(_x(), _conv(128, 256), _bn(128)) is True
        monkeypatch.setattr(bn_ops, "MLP_BF16_WIDE", False)                             # switch off
        assert not plan(_x(), _conv(128, 256), _bn(128))
        assert not plan(_x(), _conv(128, 256))
