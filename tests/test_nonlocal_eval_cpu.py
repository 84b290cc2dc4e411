"""The inference non-local route without a GPU: the three entry points are declared and exported, the float64 reference of
nonlocal_eval_cases.py (the literal (P, P) formula) equals the kernel's own algebra, the envelope query and the refusals answer
before any device call, and nonlocal_ops.nl_eval_plan decides from attributes alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nonlocal_eval_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16, SUPPORTED = "mgar_nonlocal_dot_eval_fwd", "mgar_nonlocal_dot_eval_bf16_fwd", "mgar_nonlocal_dot_eval_supported"


def test_header_declares_the_symbols():
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    for name in (FP32, BF16, SUPPORTED):
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
    assert not BF16.endswith("_bf16")                        # called by name: the count of `_bf16` payload twins stays
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert FP32 in open(os.path.join(ROOT, doc)).read(), doc
    assert "MGAR_NL_EVAL_FUSE" in open(os.path.join(ROOT, "README.md")).read()


def test_library_exports_the_symbols():
    from multimodal_gar_amd import _lib, op_timer
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(cdll, n) for n in (FP32, BF16, SUPPORTED))
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    for name in (FP32, BF16):
        assert _lib._fns[name].restype is I and list(_lib._fns[name].argtypes) == [P, LL, LL, LL, I, I, I, I, P, P, P, P, P, P, P, P]
    assert list(_lib._fns[SUPPORTED].argtypes) == [I, I, I]
    assert "mgar_nonlocal_dot_eval" not in _lib.BF16_TWINS
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "nonlocal_dot_eval" in names and len(set(names)) == len(names)
    assert op_timer.KERNEL_SOURCES.get("nonlocal_dot_eval") == "nonlocal_eval.hip"
    assert os.path.exists(os.path.join(ROOT, "multimodal_gar_amd", "csrc", "nonlocal_eval.hip"))


def test_envelope_and_refusals_without_a_device():
    """Every (Ci, P) of the issue's envelope is supported at the smallest and the largest C; one step outside is not; the entry
    points refuse before any device call (this machine has none)."""
    from multimodal_gar_amd import _lib
    sup = _lib._fns[SUPPORTED]
    for c in (1, 1024):
        assert all(sup(c, ci, p) == 1 for ci in range(1, 129) for p in range(1, min(256, 4096 // ci) + 1))
    for case in N.CASES:
        assert sup(*case[1:]) == 1
    for bad in ((8, 2, 257), (8, 129, 1), (8, 17, 241), (1025, 2, 9), (0, 1, 1), (8, 0, 9), (8, 2, 0), (-1, 2, 9)):
        assert sup(*bad) == 0, bad
    for name in (FP32, BF16):
        f = _lib._fns[name]
        nul = (None,) * 8
        assert f(None, 18, 9, 1, 4, 8, 2, 257, *nul) == -3 and f(None, 1, 1, 1, 4, 8, 129, 1, *nul) == -3        # MGAR_EUNSUPPORTED
        assert f(None, 241 * 8, 241, 1, 4, 8, 17, 241, *nul) == -3
        assert f(None, 18, 9, 1, 4, 8, 2, 9, *nul) == -1 and b"null" in _lib._cdll.mgar_last_error()             # MGAR_EINVAL
        assert f(None, 18, 9, 1, -1, 8, 2, 9, *nul) == -1 and f(None, 18, 9, 1, 4, 0, 2, 9, *nul) == -1
        assert f(None, 18, -9, 1, 4, 8, 2, 9, *nul) == -1
        assert f(None, 18, 9, 1, 0, 8, 2, 9, *nul) == 0                                                          # n == 0: MGAR_OK


@pytest.mark.parametrize("bn_layer", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("case", [c for c in N.CASES if c[0] * c[1] * c[3] <= 80000], ids=N.case_id)
def test_literal_reference_equals_the_factored_form(case, bn_layer):
    """The test's own reference: the literal float64 formula (the (P, P) matrix) equals S = G Phi^T / P, Y = S T with the
    folded affine map to 1e-12; the bound is positive and finite, and K counts what the issue says."""
    ref, bound = N.reference(case, bn_layer, False)
    alt = N.factored(case, bn_layer, N.make_x(case))
    assert ref.shape == alt.shape == (case[0], case[1], case[3])
    assert np.abs(ref - alt).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.isfinite(bound).all() and (bound > 0).all()
    mag = bound / ((case[1] + case[3] + 2 * case[2] + 8) * N.U)
    assert (mag >= np.abs(ref) * (1 - 1e-12)).all()                     # |chain(x)| <= chain(|x|)
    refb, boundb = N.reference(case, bn_layer, True)
    x16 = N.make_x(case, True)
    assert np.array_equal(N.to_bf16(x16), x16) and not np.array_equal(x16, N.make_x(case))
    assert (boundb >= N.BF16_EPS * np.abs(refb)).all()


def test_the_module_and_the_cases_agree():
    """make_block's eval forward (the torch route, on the host) equals the float64 reference inside the fp32 bound: the case
    parameters are the module's."""
    case = (3, 32, 4, 25)
    for bn_layer in (True, False):
        blk = N.make_block(case, bn_layer)
        with torch.no_grad():
            got = blk(torch.from_numpy(N.make_x(case).copy())).double().numpy()
        ref, bound = N.reference(case, bn_layer, False)
        assert (np.abs(got - ref) <= bound).all()


def test_plan_decisions_without_a_device(monkeypatch):
    from multimodal_gar_amd import nonlocal_ops as O
    from multimodal_gar_amd.model.backbone import NLBlockND
    monkeypatch.setattr(O, "NL_EVAL_FUSE", True)
    x = torch.randn(2, 32, 5, 5)
    with torch.no_grad():
        for mode in ("embedded", "gaussian", "concatenate"):
            blk = NLBlockND(32, 4, mode=mode, dimension=2).eval()
            assert O.nl_eval_refusal(blk, x) == "mode" and O.nl_eval_plan(blk, x) is None
        blk = NLBlockND(32, 4, mode="dot", dimension=2).eval()
        assert O.nl_eval_refusal(blk, x) == "device" and O.nl_eval_plan(blk, x) is None           # a host tensor: everything else holds
        assert O.nl_eval_refusal(blk, x.flatten(2).permute(0, 2, 1), rows=True) == "device"
        assert O.nl_eval_refusal(blk, x.double()) == "payload" and O.nl_eval_refusal(blk, x.half()) == "payload"
        assert O.nl_eval_refusal(blk, torch.randn(2, 32, 17, 17)) == "size"                       # P = 289
        assert O.nl_eval_refusal(blk, torch.randn(2, 16, 5, 5)) == "size"                         # not the block's channels
        assert O.nl_eval_refusal(blk.train(), x) == "batch norm"                                  # a training BatchNorm
        blk.eval()
        blk.W_z[1].train()
        assert O.nl_eval_refusal(blk, x) == "batch norm"
        blk.eval()
        nostat = NLBlockND(32, 4, mode="dot", dimension=2)
        nostat.W_z[1] = torch.nn.BatchNorm2d(32, track_running_stats=False)
        assert O.nl_eval_refusal(nostat.eval(), x) == "batch norm"
        h = blk.theta.register_forward_hook(lambda m, a, o: None)
        assert O.nl_eval_refusal(blk, x) == "hook"
        h.remove()
        assert O.nl_eval_refusal(NLBlockND(32, 4, mode="dot", dimension=2, bn_layer=False).train(), x) == "device"   # no BatchNorm at all
        monkeypatch.setattr(O, "NL_EVAL_FUSE", False)
        assert O.nl_eval_refusal(blk, x) == "switch off" and O.nl_eval_plan(blk, x) is None
        monkeypatch.setattr(O, "NL_EVAL_FUSE", True)
    assert O.nl_eval_refusal(blk, x) == "gradient"                                                # grad mode on, parameters want one
    for q in blk.parameters():
        q.requires_grad_(False)
    assert O.nl_eval_refusal(blk, x) == "device"
    assert O.nl_eval_refusal(blk, x.clone().requires_grad_(True)) == "gradient"                   # a grad-requiring input
    with torch.no_grad():
        assert O.nl_eval_refusal(blk, x.clone().requires_grad_(True)) == "device"
    # the torch route is what runs on the host, and forward_rows feeds it the same values
    with torch.no_grad():
        y = blk(x)
        assert torch.equal(blk.forward_rows(x.flatten(2).permute(0, 2, 1).contiguous()), y.flatten(2))


def test_switch_reads_the_environment():
    import subprocess
    import sys
    code = "from multimodal_gar_amd import nonlocal_ops; print(nonlocal_ops.NL_EVAL_FUSE)"
    env = dict(os.environ, MGAR_NL_EVAL_FUSE="0")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "False"


def test_params_are_cached_by_tensor_version():
    """The stacked weights and the affine pair are built once for a frozen block and rebuilt after an in-place update."""
    from multimodal_gar_amd import nonlocal_ops as O
    for bn_layer in (True, False):
        blk = N.make_block((3, 32, 4, 25), bn_layer)
        parts = O._parts(blk)
        a, b = O._params(blk, parts), O._params(blk, parts)
        assert all(s is t for s, t in zip(a, b))
        p = N.params((3, 32, 4, 25), bn_layer)
        for got, key in zip(a, ("w_tpg", "b_tpg", "w_z", "b_z", "scale", "shift")):
            assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == p[key].shape
            if key in ("scale", "shift"):       # sparse_ops.fold_bn forms rsqrt * gamma, the cases gamma / sqrt: one fp32 ulp apart at most
                assert np.allclose(got.numpy(), p[key], rtol=2.0 ** -23, atol=0.0), key
            else:
                assert np.array_equal(got.numpy(), p[key]), key
        with torch.no_grad():
            blk.phi.weight.mul_(2.0)
        c = O._params(blk, parts)
        assert c[0] is not a[0] and torch.equal(c[0][4:8], 2.0 * a[0][4:8]) and torch.equal(c[0][:4], a[0][:4])
        if bn_layer:
            with torch.no_grad():
                blk.W_z[1].running_var.add_(1.0)
            d = O._params(blk, parts)
            assert d[4] is not c[4] and not torch.equal(d[4], c[4]) and d[0] is not c[0]
