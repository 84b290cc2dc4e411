"""csrc/scene_ops.hip through the C ABI (multimodal_gar_amd/scene_ops.py binds nothing else) against the float64 references
and rounding-count bounds of tests/scene_cases.py, which tests/test_scene_ops_cpu.py shows to be satisfiable and to bite."""
import ctypes

import numpy as np
import pytest
import torch

import scene_cases as SC

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype=dtype)


def _bn_run(case, inp):
    from multimodal_gar_amd import scene_ops as SO
    from multimodal_gar_amd.dafm_ops import scene_offsets
    so, _ = scene_offsets(case["counts"], "cuda")
    x, gamma, beta = (_dev(inp[k]).requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = _dev(inp["running_mean"]), _dev(inp["running_var"])
    nbt = torch.tensor(inp["num_batches_tracked"], dtype=torch.int64, device="cuda")
    y = SO.scene_batch_norm(x, gamma, beta, so, rm, rv, nbt, SC.BN_EPS, SC.BN_MOMENTUM)
    y.backward(_dev(inp["dy"]))
    return dict(y=y.detach(), running_mean=rm, running_var=rv, nbt=int(nbt.item()), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.parametrize("name", list(SC.BN_CASES))
def test_scene_bn_case(name):
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import scene_offsets
    case = SC.BN_CASES[name]
    counts, inp = case["counts"], SC.bn_inputs(case)
    ref = SC.bn_ref(counts, inp)
    got = _bn_run(case, inp)
    for what in ("y", "running_mean", "running_var", "dx", "dgamma", "dbeta"):
        r = SC.worst_ratio(got[what].cpu().numpy(), ref, what)
        print("%s %s: err / bound %.3g" % (name, what, r))
        assert r <= 1.0, (what, r)
    assert got["nbt"] == inp["num_batches_tracked"] + ref["steps"]
    # the saved statistics, straight from the entry point (no running statistics: NULL is allowed)
    S, C, rows = len(counts), case["C"], sum(counts)
    so, _ = scene_offsets(counts, "cuda")
    x, gamma, beta = _dev(inp["x"]), _dev(inp["gamma"]), _dev(inp["beta"])
    y = torch.full_like(x, float("nan"))
    mean, invstd, var = (torch.full((S, C), float("nan"), device="cuda") for _ in range(3))
    L.call("mgar_scene_bn_fwd", S, rows, C, L.iptr(so), L.fptr(x), L.fptr(gamma), L.fptr(beta), SC.BN_EPS, SC.BN_MOMENTUM, None,
           None, None, L.fptr(y), L.fptr(mean), L.fptr(invstd), L.fptr(var), L.stream_of(x))
    assert torch.equal(y, got["y"])
    full = np.array([n >= 2 for n in counts])
    for what, t in (("mean", mean), ("var", var), ("invstd", invstd)):
        a = t.cpu().numpy()
        assert np.isfinite(a).all()
        sub = {what: ref[what][full], what + "_bound": ref[what + "_bound"][full]}
        assert SC.worst_ratio(a[full], sub, what) <= 1.0, what
    for s, n in enumerate(counts):                       # a one-row scene: y = beta exactly, no gradient to x
        if n == 1:
            r = int(sum(counts[:s]))
            assert torch.equal(got["y"][r], beta) and not got["dx"][r].any()
    # three runs give equal bits
    for _ in range(2):
        again = _bn_run(case, inp)
        for what in ("y", "running_mean", "running_var", "dx", "dgamma", "dbeta"):
            assert torch.equal(again[what], got[what]), what


def test_scene_bn_writes_nothing_outside_its_rows():
    """Guard rows around x / y and an empty scene between two others: the kernels touch the scenes' rows only."""
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import scene_offsets
    counts, C = [3, 0, 1, 4], 64
    rows = sum(counts)
    so, _ = scene_offsets(counts, "cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(rows, C, device="cuda", generator=g)
    buf = torch.full((rows + 2, C), 7.0, device="cuda")
    y = buf[1:-1]
    mean, invstd, var = (torch.empty(len(counts), C, device="cuda") for _ in range(3))
    w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    L.call("mgar_scene_bn_fwd", len(counts), rows, C, L.iptr(so), L.fptr(x), L.fptr(w), L.fptr(b), 1e-5, 0.1, None, None, None,
           y.data_ptr(), L.fptr(mean), L.fptr(invstd), L.fptr(var), L.stream_of(x))
    assert (buf[0] == 7).all() and (buf[-1] == 7).all() and not (buf[1:-1] == 7).any()


@pytest.mark.parametrize("name", list(SC.GEOM_CASES))
def test_pair_geometry_case(name):
    """De within one fp32 ulp of the float64 restatement (1e-6 absolute on the clamped entries); Dg within twice what
    torch's own fp32 _giou_batched (on the CPU) differs from float64 on the same boxes, scene by scene --
    measured 1.5e-7, so the bound is 3.0e-7."""
    from multimodal_gar_amd import scene_ops as SO
    from multimodal_gar_amd.dafm_ops import scene_offsets
    centres, boxes = SC.geom_inputs(SC.GEOM_CASES[name])
    so, do, pairs = SC.offsets(SC.GEOM_COUNTS)
    dso, ddo = scene_offsets(SC.GEOM_COUNTS, "cuda")
    de, dg = SO.scene_pair_geometry(_dev(centres), _dev(boxes), dso, ddo, pairs)
    de2, none = SO.scene_pair_geometry(_dev(centres), None, dso, ddo, pairs)
    assert none is None and torch.equal(de, de2)
    de, dg = de.cpu().numpy(), dg.cpu().numpy()
    for s, n in enumerate(SC.GEOM_COUNTS):
        if n == 0:
            continue
        c, b = centres[so[s]:so[s + 1]], boxes[so[s]:so[s + 1]]
        got = de[do[s]:do[s] + n * n].reshape(n, n)
        ok, de_err = SC.de_close(got, SC.de_ref(c))
        assert ok, (s, n, de_err)
        assert not np.diag(got).any()
        g64 = SC.giou(b, np.float64)
        bound = 2 * SC.giou_fp32_error(b)
        err = np.abs(dg[do[s]:do[s] + n * n].reshape(n, n).astype(np.float64) - g64).max()
        print("%s scene %d n %d: De err %.3g, Dg err %.3g bound %.3g" % (name, s, n, de_err, err, bound))
        assert err <= bound, (s, n, err, bound)


@pytest.mark.parametrize("name", list(SC.GRAM_CASES))
def test_scene_gram_case(name):
    from multimodal_gar_amd import scene_ops as SO
    from multimodal_gar_amd.dafm_ops import scene_offsets
    case = SC.GRAM_CASES[name]
    counts = case["counts"]
    x0, dg0 = SC.gram_inputs(case)
    ref = SC.gram_ref(counts, x0, dg0)
    so, do = scene_offsets(counts, "cuda")
    x = _dev(x0).requires_grad_(True)
    g = SO.scene_gram(x, so, do, dg0.size)
    g.backward(_dev(dg0))
    for what, t in (("g", g.detach()), ("dx", x.grad)):
        r = SC.worst_ratio(t.cpu().numpy(), ref, what)
        print("%s %s: err / bound %.3g" % (name, what, r))
        assert r <= 1.0, (what, r)
    hso, hdo, _ = SC.offsets(counts)
    for s, n in enumerate(counts):                       # one chain per entry, the same for (i, j) and (j, i)
        blk = g.detach()[hdo[s]:hdo[s] + n * n].view(n, n)
        assert torch.equal(blk, blk.T)


def test_argument_checks_come_before_any_launch():
    """Null pointers and negative sizes: MGAR_EINVAL; a channel count that is no multiple of 64: MGAR_EUNSUPPORTED; no scene
    or no row: MGAR_OK.  All with pointers that a launch would fault on or buffers it would overwrite."""
    from multimodal_gar_amd import _lib as L
    EINVAL, EUNSUP = -1, -3
    t = torch.full((64, 64), 5.0, device="cuda")
    p, st = t.data_ptr(), L.stream_of(t)
    i32 = torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr()
    f = ctypes.c_float
    bn_f = lambda S, rows, C, so=i32, x=p, y=p: L.raw("mgar_scene_bn_fwd", S, rows, C, so, x, p, p, f(1e-5), f(0.1), None, None, None,
                                                     y, p, p, p, st)
    bn_b = lambda S, rows, C, gx=p: L.raw("mgar_scene_bn_bwd", S, rows, C, i32, p, p, p, p, p, p, gx, p, p, st)
    geo = lambda S, rows, de=p, boxes=None, dg=None: L.raw("mgar_scene_pair_geometry", S, rows, i32, i32, p, boxes, de, dg, st)
    gr_f = lambda S, rows, D, g=p: L.raw("mgar_scene_gram_fwd", S, rows, D, i32, i32, p, g, st)
    gr_b = lambda S, rows, D, gx=p: L.raw("mgar_scene_gram_bwd", S, rows, D, i32, i32, p, p, gx, st)
    assert bn_f(-1, 4, 64) == EINVAL and bn_f(1, -4, 64) == EINVAL and bn_f(1, 4, 0) == EINVAL and bn_f(1, 4, -64) == EINVAL
    assert bn_f(1, 4, 64, so=None) == EINVAL and bn_f(1, 4, 64, x=None) == EINVAL and bn_f(1, 4, 64, y=None) == EINVAL
    assert bn_f(1, 4, 96) == EUNSUP and bn_f(1, 4, 32) == EUNSUP
    assert bn_f(0, 0, 64) == 0 and bn_f(3, 0, 64) == 0
    assert bn_b(-1, 4, 64) == EINVAL and bn_b(1, 4, 64, gx=None) == EINVAL and bn_b(1, 4, 100) == EUNSUP and bn_b(0, 0, 64) == 0
    assert geo(-1, 4) == EINVAL and geo(1, -1) == EINVAL and geo(1, 4, de=None) == EINVAL and geo(1, 4, boxes=p, dg=None) == EINVAL
    assert geo(0, 0) == 0 and geo(2, 0) == 0
    assert gr_f(-1, 4, 64) == EINVAL and gr_f(1, 4, 0) == EINVAL and gr_f(1, 4, 64, g=None) == EINVAL and gr_f(1, 4, 65) == EUNSUP
    assert gr_f(0, 0, 64) == 0
    assert gr_b(1, -4, 64) == EINVAL and gr_b(1, 4, 64, gx=None) == EINVAL and gr_b(1, 4, 72) == EUNSUP and gr_b(0, 0, 64) == 0
    assert b"multiple of 64" in L.raw("mgar_last_error")
    torch.cuda.synchronize()
    assert (t == 5).all()                                # nothing ran
