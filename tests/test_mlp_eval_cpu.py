"""The inference shared-MLP route without a GPU: the two entry points (mgar_pointwise_conv_maxpool_eval_fwd,
mgar_pointwise_conv_maxpool_eval_bf16_fwd) are declared, exported and bound with the header's prototypes, and refuse unsupported
shapes before any device call; the bound of the device test (mlp_eval_cases.py) is satisfiable by a correct fp32 evaluation and
five wrong restatements of the kernel leave it; the cases exercise what they claim (decided from the float64 reference alone);
and the routing predicate bn_ops.eval_mlp_plan decides from attributes only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_eval_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16 = "mgar_pointwise_conv_maxpool_eval_fwd", "mgar_pointwise_conv_maxpool_eval_bf16_fwd"
MGAR_OK, MGAR_EINVAL, MGAR_EUNSUPPORTED = 0, -1, -3
SMALL_IDS = [E.case_id(c) for c in E.SMALL_CASES]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_symbols():
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    I, P = ctypes.c_int, ctypes.c_void_p
    #      x  B  Cin M ns w  rs cs Cout mean invstd gamma beta in_relu scale shift out_relu pooled stream
    want = [P, I, I, I, I, P, I, I, I, P, P, P, P, I, P, P, I, P, P]
    for name in (FP32, BF16):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
        assert name in _lib.exported_symbols()
        assert _lib._fns[name].restype is I and list(_lib._fns[name].argtypes) == want, name
    # called by name: neither is in the table of `_bf16` payload twins, whose size existing tests pin
    assert FP32 not in _lib.BF16_TWINS and not BF16.endswith("_bf16") and len(_lib.BF16_TWINS) == 27
    assert _lib.ABI_VERSION >= 21
    assert cdll.mgar_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("name", [FP32, BF16])
def test_entries_refuse_before_any_device_call(name):
    from multimodal_gar_amd import _lib
    fn = _lib._fns[name]
    one = ctypes.c_void_p(16)                      # non-null, aligned, never dereferenced: every call below fails first

    def call(B=2, Cin=8, M=5, ns=16, Cout=8, x=one, w=one, scale=one, shift=one, pooled=one, mean=None, invstd=None):
        return fn(x, B, Cin, M, ns, w, Cin, 1, Cout, mean, invstd, None, None, 1, scale, shift, 1, pooled, None)

    for kw in (dict(ns=24), dict(Cout=65), dict(ns=6), dict(ns=1), dict(ns=256), dict(ns=12), dict(Cin=257), dict(Cin=0)):
        assert call(**kw) == MGAR_EUNSUPPORTED, kw
        assert b"pointwise_conv_maxpool_eval" in _lib._cdll.mgar_last_error()
    for kw in (dict(B=-1), dict(M=-1), dict(ns=0), dict(Cin=-1), dict(Cout=-1), dict(M=1 << 26, ns=32)):
        assert call(**kw) == MGAR_EINVAL, kw
    for kw in (dict(x=None), dict(w=None), dict(scale=None), dict(shift=None), dict(pooled=None), dict(mean=one)):
        assert call(**kw) == MGAR_EINVAL, kw
    for kw in (dict(B=0), dict(M=0), dict(Cout=0)):    # nothing to do: MGAR_OK without touching a pointer
        assert call(x=None, w=None, pooled=None, **kw) == MGAR_OK, kw


# ---- the bound and the cases ------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_the_issue_names():
    shapes = [c[0] for c in E.CASES]
    assert {s[4] for s in shapes if s[1] <= 16 and s[2] <= 16 and s[0] == 2} >= set(E.NSAMPLES)
    assert any(s[3] * s[4] % 128 for s in shapes)
    assert {(s[2], s[1]) for s in shapes} >= {(co, ci) for co in (1, 7, 32, 33, 64) for ci in (1, 3, 16, 17, 64)}
    assert any(s[0] * -(-s[3] * s[4] // 128) > 8192 for s in shapes)
    assert {c[1] for c in E.CASES} == {"bn", "noaffine", "id"}
    assert {(c[2], c[3]) for c in E.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for c in E.CASES:
        assert c[0][4] in E.NSAMPLES and 1 <= c[0][1] <= 256 and c[0][2] <= 64


@pytest.mark.parametrize("ns", E.NSAMPLES)
def test_argmax_reaches_every_lane_and_component(ns):
    """In the reference the arg-max of a group falls, with a margin above twice the bound, at least once at every lane position
    s // 4 of the group and at every in-lane component s % 4: a shuffle step or a component the kernel dropped cannot hide."""
    seen = E.argmax_coverage(E.SMALL_CASES, ns)
    assert {s // 4 for s in seen} == set(range(ns // 4)), ns
    assert {s % 4 for s in seen} == {0, 1, 2, 3}, ns


@pytest.mark.parametrize("case", E.CASES, ids=[E.case_id(c) for c in E.CASES])
def test_generator_conditions(case):
    d = E.make_case(case)
    ref, lim, v, _ = E.reference(case)
    cout = case[0][2]
    assert np.isfinite(ref).all() and (lim > 0).all()
    if cout > 1:
        assert (d["scale"] > 0).any() and (d["scale"] < 0).any()
        assert len(np.unique(d["scale"])) == cout and len(np.unique(d["shift"])) == cout
    if cout > 2:
        assert (d["shift"] > 0).any() and (d["shift"] < 0).any()
    if d["out_relu"]:
        assert (ref == 0).any() and (ref > 0).any()            # whole groups are cut to 0, others are not
        assert (v == 0).any() and not np.signbit(ref).any()
    else:
        assert (ref < 0).any() or cout == 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", E.CASES, ids=[E.case_id(c) for c in E.CASES])
def test_fp32_restatement_is_inside_the_bound(case, bf16):
    """A correct fp32 evaluation (sequential fma chain) uses at most 0.29 of the fp32 bound and 0.99 of the bf16 bound (one
    rounding at 2^-8 relative, attained next to a power of two)."""
    got = E.emulate(case, bf16)
    u = E.used(got, case, bf16)
    print("%s %s: max err / bound = %.3f" % (E.case_id(case), "bf16" if bf16 else "fp32", u))
    assert u <= 1.0


def _applies(case, mutant):
    (_, _, cout, _, _), _, _, out_relu = case
    return {"scale_xor1": cout >= 2, "relu_first": bool(out_relu)}.get(mutant, True)


@pytest.mark.parametrize("mutant", ["scale_xor1", "relu_first", "half_group", "no_shift"])
def test_wrong_restatements_leave_the_bound(mutant):
    """scale taken at o ^ 1, ReLU before the affine, max over half the group, shift dropped: each leaves the bound at EVERY case
    it can differ at (scale_xor1: Cout >= 2; relu_first: out_relu)."""
    cases = [c for c in E.SMALL_CASES if _applies(c, mutant)]
    assert len(cases) >= 12
    for case in cases:
        u = E.used(E.emulate(case, False, mutant), case, False)
        assert u > 1.0, (mutant, E.case_id(case), u)


def test_bf16_rounded_early_leaves_the_bound():
    """bf16: the conv output rounded before the affine and the max (the unfused route's second rounding) leaves the bound of a
    single rounding wherever scale z and shift cancel: at every case with Cout >= 7 here.  (Rounding v itself before the max is
    the same function as rounding after it -- rounding to nearest is monotone -- so no test can tell those apart.)"""
    cases = [c for c in E.SMALL_CASES if c[0][2] >= 7]
    assert len(cases) >= 20
    for case in cases:
        u = E.used(E.emulate(case, True, "bf16_early"), case, True)
        assert u > 1.0, (E.case_id(case), u)
    v = np.float32([1.00390625, 1.0078125, -3.0, 0.5])
    assert E.to_bf16(v).max() == E.to_bf16(v.max())


# ---- the routing predicate --------------------------------------------------------------------------------------------------------
class _Attr:
    """What eval_mlp_plan may look at in a tensor: attributes.  Anything that would read or synchronise raises."""

    def __init__(self, shape, dtype=torch.float32, is_cuda=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, is_cuda, requires_grad

    def dim(self):
        return len(self.shape)

    def __getattr__(self, name):
        raise AssertionError("eval_mlp_plan touched tensor.%s" % name)


def _layers(cin=32, cout=64, bias=False, conv_cls=nn.Conv2d):
    bn, conv, bn2 = nn.BatchNorm2d(cin), conv_cls(cin, cout, kernel_size=1, bias=bias), nn.BatchNorm2d(cout)
    for m in (bn, conv, bn2):
        m.eval()
        for p in m.parameters():
            p.requires_grad_(False)
    return bn, conv, bn2


def test_plan_true_cases(monkeypatch):
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    bn, conv, bn2 = _layers()
    relu = nn.ReLU()
    x = _Attr((1, 32, 2048, 32))
    assert bn_ops.eval_mlp_plan(x, bn, conv, bn2, (relu,)) == "conv_maxpool"
    assert bn_ops.eval_mlp_plan(x, None, conv, bn2) == "conv_maxpool"                # identity prologue
    assert bn_ops.eval_mlp_plan(x, bn, conv) == "conv"
    assert bn_ops.eval_mlp_plan(_Attr((1, 32, 2048, 32), torch.bfloat16), bn, conv, bn2) == "conv_maxpool"
    with torch.no_grad():                                                            # grad mode off: parameters may want one
        conv.weight.requires_grad_(True)
        assert bn_ops.eval_mlp_plan(_Attr((1, 32, 2048, 32), requires_grad=True), bn, conv, bn2) == "conv_maxpool"
    conv.weight.requires_grad_(False)
    for ns in E.NSAMPLES:
        assert bn_ops.eval_mlp_plan(_Attr((1, 32, 65536 // ns, ns)), bn, conv, bn2) == "conv_maxpool", ns
    b256, c256, _ = _layers(256, 64)
    assert bn_ops.eval_mlp_plan(_Attr((1, 256, 2048, 32)), b256, c256, bn2) == "conv_maxpool"
    assert bn_ops.eval_mlp_plan(_Attr((1, 256, 2048, 32)), b256, c256) is None       # the plain step keeps C <= 64


def test_plan_every_refusal(monkeypatch):
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    x = _Attr((1, 32, 2048, 32))

    def plan(x=x, edit=None, pool=True, **kw):
        bn, conv, bn2 = _layers(**kw)
        relu = nn.ReLU()
        if edit:
            edit(bn, conv, bn2, relu)
        return bn_ops.eval_mlp_plan(x, bn, conv, bn2 if pool else None, (relu,))

    assert plan() == "conv_maxpool" and plan(pool=False) == "conv"
    assert plan(edit=lambda bn, conv, bn2, relu: bn.train()) is None                                  # training BatchNorm, either
    assert plan(edit=lambda bn, conv, bn2, relu: bn2.train()) is None
    assert plan(edit=lambda bn, conv, bn2, relu: bn.train(), pool=False) is None
    assert plan(edit=lambda bn, conv, bn2, relu: conv.weight.requires_grad_(True)) is None            # a required gradient
    assert plan(edit=lambda bn, conv, bn2, relu: bn2.bias.requires_grad_(True)) is None
    assert plan(x=_Attr((1, 32, 2048, 32), requires_grad=True)) is None
    assert plan(edit=lambda bn, conv, bn2, relu: conv.register_forward_hook(lambda *a: None)) is None  # a hook, anywhere
    assert plan(edit=lambda bn, conv, bn2, relu: bn2.register_forward_pre_hook(lambda *a: None)) is None
    assert plan(edit=lambda bn, conv, bn2, relu: relu.register_forward_hook(lambda *a: None)) is None
    assert plan(x=_Attr((1, 32, 4096, 24))) is None                                                   # ns = 24
    assert plan(x=_Attr((1, 32, 4096, 24)), pool=False) == "conv"                                     # ... the plain step takes it
    assert plan(x=_Attr((1, 32, 1024, 256))) is None
    assert plan(cout=128) is None and plan(cout=128, pool=False) is None                              # Cout = 128
    assert plan(cin=65, cout=64, x=_Attr((1, 65, 2048, 32)), pool=False) is None
    assert plan(bias=True) is None and plan(bias=True, pool=False) is None                            # a bias
    assert plan(x=_Attr((1, 32, 2047, 32))) is None                                                   # B * P < 65 536
    assert plan(x=_Attr((1, 32, 2048, 32), is_cuda=False)) is None                                    # not on the device
    assert plan(x=_Attr((1, 32, 2048, 32), torch.float16)) is None
    assert plan(x=_Attr((1, 16, 2048, 32))) is None                                                   # channels do not match
    assert plan(x=_Attr((1, 32, 65536)), conv_cls=nn.Conv1d) is None                                  # pooling needs (B, C, M, ns)
    assert plan(edit=lambda bn, conv, bn2, relu: setattr(bn2, "running_mean", None)) is None          # no running statistics

    def not_pointwise(bn, conv, bn2, relu):
        conv.stride = (2, 1)
    assert plan(edit=not_pointwise) is None
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", False)                                               # the switch
    assert plan() is None and plan(pool=False) is None


def test_switch_reads_the_environment():
    import subprocess
    import sys
    code = "from multimodal_gar_amd import bn_ops; print(bn_ops.MLP_EVAL_FUSE)"
    env = dict(os.environ, MGAR_MLP_EVAL_FUSE="0")       # one child process: the default (on) is what every other test runs under
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False", out
