"""The I3D entry points of csrc/pointwise_wide_bf16.hip on the device: mgar_conv1x1_bf16_fwd and mgar_conv1x1_bf16_fwd_affine against the float64 references and
the bounds of tests/conv1x1_bf16_cases.py, a strided channel-slice destination, batch independence, repeatability, non-finite
values and the refusals; then the routing of Unit3D / InceptionModule / InceptionI3d for bf16 payloads in train and eval mode."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv1x1_bf16_cases as K
from conftest import record_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PLAIN, AFFINE = "mgar_conv1x1_bf16_fwd", "mgar_conv1x1_bf16_fwd_affine"
K3_AFFINE, STEM_AFFINE = "mgar_conv3d_k3_bf16_fwd_affine", "mgar_stem_conv3d_bf16_fwd_affine"
EUNSUPPORTED = -3


def run(x, w, epilogue=None, y=None, bstride=None):
    """x (N, Cin, P) bf16 and w (Cout, Cin) fp32 on the device; epilogue None (the plain entry) or (scale, shift, relu);
    y / bstride: a destination slice"""
    from multimodal_gar_amd import _lib as L
    n, cin, p = x.shape
    cout = w.shape[0]
    out = torch.empty((n, cout, p), dtype=BF, device=x.device) if y is None else y
    bs = cout * p if bstride is None else bstride
    if epilogue is None:
        L.call(PLAIN, L.pptr(x, BF), n, cin, p, L.fptr(w), cout, out.data_ptr(), bs, L.stream_of(x))
    else:
        s, h, relu = epilogue
        L.call(AFFINE, L.pptr(x, BF), n, cin, p, L.fptr(w), cout, L.fptr(s), L.fptr(h), int(relu), out.data_ptr(), bs, L.stream_of(x))
    return out


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def device_case(case):
    """the case with its operands on the device and the outputs of the three calls (computed once, shared, never modified)"""
    e = dict(K.expected(case))
    e["xg"], e["wg"] = e["x"].cuda().to(BF), e["w"].cuda()
    e["sg"], e["hg"] = torch.from_numpy(np.array(e["scale"])).cuda(), torch.from_numpy(np.array(e["shift"])).cuda()
    e["plain"] = run(e["xg"], e["wg"])
    for relu in (0, 1):
        e["affine", relu] = run(e["xg"], e["wg"], (e["sg"], e["hg"], relu))
    return e


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---- the entry points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_both_entries_within_the_float64_bounds(case):
    e = device_case(case)
    used = K.plain_share(e["plain"].float().cpu(), case)
    record_error("conv1x1 bf16 plain err / bound", used, 1.0, 1.0)
    print("plain %s: %.3f of the bound" % (K.case_id(case), used))
    shares = [used]
    for relu in (0, 1):
        got = _np(e["affine", relu])
        u = K.affine_share(got, case, relu)
        record_error("conv1x1 bf16 affine relu=%d err / bound" % relu, u, 1.0, 1.0)
        print("affine relu=%d %s: %.3f of the bound" % (relu, K.case_id(case), u))
        shares.append(u)
        if relu:
            assert (got >= 0).all() and not np.signbit(got).any()                   # a negative or -0 pre-activation gives +0
    assert max(shares) <= 1.0, shares


@pytest.mark.parametrize("case", [K.CASES[2], K.CASES[3], K.CASES[5]], ids=K.case_id)
def test_writes_a_channel_slice_and_nothing_else(case):
    n, cin, cout, p = case
    e = device_case(case)
    c0, total = 5, cout + 12
    fill = 0x7FC1                                                                    # a NaN no kernel produces
    for name, epilogue in (("plain", None), (("affine", 1), (e["sg"], e["hg"], 1))):
        wide = torch.full((n, total, p), fill, dtype=torch.int16, device="cuda").view(BF)
        dst = wide[:, c0:c0 + cout]
        run(e["xg"], e["wg"], epilogue, y=dst, bstride=total * p)
        assert same_bits(dst, e[name])
        rest = wide.view(torch.int16).clone()
        rest[:, c0:c0 + cout] = fill
        assert bool((rest == fill).all())


def test_batch_independence():
    case = K.CASES[5]                                                               # N = 3, tiles straddle the samples
    e = device_case(case)
    for name, epilogue in (("plain", None), (("affine", 1), (e["sg"], e["hg"], 1))):
        for n in range(3):
            one = run(e["xg"][n:n + 1].contiguous(), e["wg"], epilogue)
            assert same_bits(one, e[name][n:n + 1])


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_repeatable(case):
    e = device_case(case)
    assert same_bits(run(e["xg"], e["wg"]), e["plain"])
    assert same_bits(run(e["xg"], e["wg"], (e["sg"], e["hg"], 1)), e["affine", 1])


@pytest.mark.parametrize("case", [K.CASES[1], K.CASES[5]], ids=K.case_id)
def test_non_finite_values_reach_their_own_column_only(case):
    n, cin, cout, p = case
    e = device_case(case)
    x = e["xg"].clone()
    col_nan, col_inf = (n - 1, p - 3), (0, 1)
    x[col_nan[0], cin // 2, col_nan[1]] = float("nan")
    x[col_inf[0], 3, col_inf[1]] = float("inf")
    x[col_inf[0], 5, col_inf[1]] = float("-inf")
    scale = e["sg"].clone()
    scale[1::5] = 0.25                                                              # (0 * inf would be a NaN of the epilogue's own)
    for epilogue, clean in ((None, e["plain"]), ((scale, e["hg"], 1), run(e["xg"], e["wg"], (scale, e["hg"], 1)))):
        got = run(x, e["wg"], epilogue)
        assert bool(torch.isnan(got[col_nan[0], :, col_nan[1]]).all())               # through the ReLU and the rounding
        assert not bool(torch.isfinite(got[col_inf[0], :, col_inf[1]]).all())
        mask = torch.ones((n, p), dtype=torch.bool, device="cuda")
        mask[col_nan], mask[col_inf] = False, False
        keep = mask[:, None, :].expand_as(got)
        assert torch.equal(bits(got)[keep], bits(clean)[keep])


def test_refusals_launch_nothing():
    from multimodal_gar_amd import _lib as L
    x = torch.zeros((1, 16, 64), dtype=BF, device="cuda")
    w = torch.zeros((513, 16), dtype=torch.float32, device="cuda")
    s = torch.ones((513,), dtype=torch.float32, device="cuda")
    fill = 0x7FC1
    y = torch.full((1, 513, 64 + 4), fill, dtype=torch.int16, device="cuda")
    st = L.stream_of(x)

    def both(n, cin, p, cout, yptr, bs):
        return (L.raw(PLAIN, x.data_ptr(), n, cin, p, w.data_ptr(), cout, yptr, bs, st),
                L.raw(AFFINE, x.data_ptr(), n, cin, p, w.data_ptr(), cout, s.data_ptr(), s.data_ptr(), 1, yptr, bs, st))
    assert both(1, 16, 62, 8, y.data_ptr(), 8 * 62) == (EUNSUPPORTED, EUNSUPPORTED)              # P % 4 != 0
    assert "library" in L.raw("mgar_last_error").decode()                                        # the message names the fallback
    assert both(1, 0, 64, 8, y.data_ptr(), 8 * 64) == (EUNSUPPORTED, EUNSUPPORTED)               # Cin = 0
    assert both(1, 16, 64, 513, y.data_ptr(), 513 * 64) == (EUNSUPPORTED, EUNSUPPORTED)          # Cout = 513
    assert both(1, 1025, 64, 8, y.data_ptr(), 8 * 64) == (EUNSUPPORTED, EUNSUPPORTED)            # Cin = 1025
    assert both(1, 16, 64, 8, y.data_ptr() + 2, 8 * 64) == (EUNSUPPORTED, EUNSUPPORTED)          # a misaligned y
    assert both(1, 16, 64, 8, y.data_ptr(), 8 * 64 + 2) == (EUNSUPPORTED, EUNSUPPORTED)          # a misaligned batch stride
    assert all(rc < 0 for rc in both(1, 16, 64, 8, y.data_ptr(), 8 * 64 - 4))                    # samples would overlap
    assert all(rc < 0 for rc in both(-1, 16, 64, 8, y.data_ptr(), 8 * 64))
    assert both(0, 16, 64, 8, y.data_ptr(), 8 * 64) == (0, 0) and both(1, 16, 0, 8, y.data_ptr(), 0) == (0, 0)   # nothing to do
    torch.cuda.synchronize()
    assert bool((y == fill).all())                                                               # nothing was written


# ---- Unit3D -----------------------------------------------------------------------------------------------------------------------
def _record_calls(monkeypatch):
    from multimodal_gar_amd import _lib as L
    calls, inner = [], L.call

    def recording(name, *a):
        calls.append((name, a))
        return inner(name, *a)
    monkeypatch.setattr(L, "call", recording)
    return calls


def _switches(monkeypatch, k1=True, fold=True):
    from multimodal_gar_amd.model.backbone import Unit3D
    monkeypatch.setattr(Unit3D, "gemm_1x1", True)
    monkeypatch.setattr(Unit3D, "k1_bf16", bool(k1))
    monkeypatch.setattr(Unit3D, "fold_bn_eval", bool(fold))
    return Unit3D


def _to_bf16_weights(mod):
    for m in mod.modules():
        if isinstance(m, nn.Conv3d):
            m.weight.data = m.weight.data.to(BF)
    for p in mod.parameters():
        p.requires_grad_(False)
    return mod


def _refuse_mm(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch.mm on the bf16 1x1x1 route")
    monkeypatch.setattr(torch, "mm", refuse)


def test_unit3d_routes(monkeypatch):
    Unit3D = _switches(monkeypatch)
    torch.manual_seed(5)
    u = _to_bf16_weights(fill_deterministic(Unit3D(48, 40, [1, 1, 1], name="k1"), seed=4).cuda())
    x = torch.relu(torch.randn(2, 48, 3, 4, 6, device="cuda")).to(BF)
    calls = _record_calls(monkeypatch)
    inner_mm = torch.mm
    state = {k: v.clone() for k, v in u.bn.state_dict().items()}
    with torch.no_grad():
        # train mode: the kernel, then the statistics + bn_act as before
        u.train()
        _refuse_mm(monkeypatch)
        new = u(x)
        names = [c[0] for c in calls]
        assert names[0] == PLAIN and AFFINE not in names and any(n.startswith("mgar_bn_") for n in names[1:]), names
        for autocast in (False, True):                                    # autocast on or off: the same bits
            with torch.autocast(device_type="cuda", dtype=BF, enabled=autocast):
                assert same_bits(u._conv(x), run(x.flatten(2), u.conv3d.weight.detach().float().view(40, 48)).view(2, 40, 3, 4, 6))
        monkeypatch.setattr(torch, "mm", inner_mm)
        # the switch off: torch.mm per sample, the bits of the route as it was
        _switches(monkeypatch, k1=False)
        u.bn.load_state_dict(state)
        del calls[:]
        mms = []
        monkeypatch.setattr(torch, "mm", lambda *a, **k: mms.append(1) or inner_mm(*a, **k))
        old = u(x)
        assert len(mms) == 2 and PLAIN not in [c[0] for c in calls]
        want = torch.stack([inner_mm(u.conv3d.weight.view(40, 48), x.flatten(2)[n]) for n in range(2)]).view(2, 40, 3, 4, 6)
        assert same_bits(u._conv(x), want)
        monkeypatch.setattr(torch, "mm", inner_mm)
        assert new.shape == old.shape and new.dtype == old.dtype == BF
        # eval mode: one _affine call, no BatchNorm kernel
        u.eval()
        u.bn.load_state_dict(state)
        _switches(monkeypatch)
        _refuse_mm(monkeypatch)
        del calls[:]
        fused = u(x)
        assert [c[0] for c in calls] == [AFFINE], calls
        _switches(monkeypatch, fold=False)                                 # fold off: the plain kernel + bn_act
        del calls[:]
        plain = u(x)
        names = [c[0] for c in calls]
        assert names[0] == PLAIN and AFFINE not in names and any(n.startswith("mgar_bn_") for n in names[1:]), names
        monkeypatch.setattr(torch, "mm", inner_mm)
        scale = plain.float().abs().max().item()
        err = (fused.float() - plain.float()).abs().max().item()
        record_error("Unit3D 1x1x1 eval fused vs unfused", err, scale, 2.0 ** -7)
        assert err <= 2.0 ** -7 * scale, (err, scale)
        # fp32 payloads keep the library GEMM
        _switches(monkeypatch)
        u32 = fill_deterministic(Unit3D(48, 40, [1, 1, 1], name="k1"), seed=4).cuda().eval()
        del calls[:]
        u32(x.float())
        assert not {PLAIN, AFFINE} & {c[0] for c in calls}


# ---- InceptionModule ----------------------------------------------------------------------------------------------------------------
def test_inception_module_eval_writes_every_branch_end_into_the_concatenation(monkeypatch):
    from multimodal_gar_amd.model.backbone import InceptionModule
    _switches(monkeypatch)
    torch.manual_seed(2)
    oc = [64, 96, 128, 16, 32, 32]
    mod = _to_bf16_weights(fill_deterministic(InceptionModule(192, oc, "m"), seed=8).cuda().eval())
    x = torch.relu(torch.randn(2, 192, 3, 9, 12, device="cuda")).to(BF)
    calls = _record_calls(monkeypatch)
    copies = []
    inner_copy = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: copies.append(tuple(self.shape)) or inner_copy(self, *a, **k))
    _refuse_mm(monkeypatch)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF):
        y = mod(x)
        monkeypatch.setattr(torch.Tensor, "copy_", inner_copy)
        names = [c[0] for c in calls]
        assert names.count(AFFINE) == 4 and names.count(K3_AFFINE) == 2 and not any(n.startswith("mgar_bn_") for n in names), names
        dhw, item = 3 * 9 * 12, y.element_size()
        total = oc[0] + oc[2] + oc[4] + oc[5]
        assert y.shape == (2, total, 3, 9, 12)
        k1 = [c[1] for c in calls if c[0] == AFFINE]                       # in call order: b0, b1a, b2a, b3b
        assert [a[5] for a in k1] == [oc[0], oc[1], oc[3], oc[5]]
        for a, c0 in ((k1[0], 0), (k1[3], oc[0] + oc[2] + oc[4])):          # b0 and b3b: their channels of y, y's batch stride
            assert a[9] == y.data_ptr() + c0 * dhw * item and a[10] == total * dhw
        assert copies == [], copies
    monkeypatch.undo()
    _switches(monkeypatch, k1=True, fold=False)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF):
        want = mod(x)
    scale = want.float().abs().max().item()
    err = (y.float() - want.float()).abs().max().item()
    record_error("InceptionModule bf16 eval fused vs unfused", err, scale, 2.0 ** -7)
    assert err <= 2.0 ** -7 * scale, (err, scale)


# ---- the trunk ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunk16():
    from multimodal_gar_amd.model.backbone import InceptionI3d
    torch.manual_seed(21)
    net = InceptionI3d(final_endpoint="Mixed_4f")
    net.build()
    net = _to_bf16_weights(fill_deterministic(net, seed=6).eval())
    x = torch.randn(2, 3, 5, 32, 64, generator=torch.Generator().manual_seed(1))
    return net.cuda(), x.cuda()


def _features(net, x):
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF):
        return net.extract_features(x)


def test_bf16_eval_trunk_runs_no_library_gemm_and_no_batchnorm_kernel(monkeypatch):
    net, x = _trunk16()
    _switches(monkeypatch)
    calls = _record_calls(monkeypatch)
    _refuse_mm(monkeypatch)
    y = _features(net, x)
    names = [c[0] for c in calls]
    assert y.dtype == BF and bool(torch.isfinite(y).all())
    assert not any(n.startswith("mgar_bn_") for n in names), sorted(set(names))
    assert names.count(AFFINE) == 29 and names.count(K3_AFFINE) + names.count(STEM_AFFINE) == 16
    assert PLAIN not in names


def test_bf16_train_mode_trunk_runs_no_library_gemm(monkeypatch):
    net, x = _trunk16()
    net = copy.deepcopy(net).train()
    _switches(monkeypatch)
    calls = _record_calls(monkeypatch)
    _refuse_mm(monkeypatch)
    y = _features(net, x)
    names = [c[0] for c in calls]
    assert y.dtype == BF and names.count(PLAIN) == 29 and AFFINE not in names


def test_bf16_eval_trunk_graph_replay_equals_eager(monkeypatch):
    net, x = _trunk16()
    _switches(monkeypatch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _features(net, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = _features(net, x).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _features(net, x)
    graph.replay()
    first = out.clone()
    graph.replay()
    second = out.clone()
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    assert torch.equal(first, eager), "replay differs from eager: max |diff| %g" % (first.float() - eager.float()).abs().max().item()
