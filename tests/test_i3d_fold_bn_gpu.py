"""The eval-mode BatchNorm [+ ReLU] store of the dense I3D convolutions on the device: mgar_conv3d_k3_fwd_affine,
mgar_conv3d_k3_bf16_fwd_affine, mgar_stem_conv3d_fwd_affine and mgar_stem_conv3d_bf16_fwd_affine against the plain entries
(identity, epilogue exactness), the float64 references and per-element bounds of tests/i3d_fold_bn_cases.py, a strided channel-slice
destination, repeatability, batch independence and NaN propagation; then the routing of Unit3D / InceptionModule / InceptionI3d
in eval mode, and eval-mode inference of several clips in one pass (InceptionI3d and the whole ClipModel)."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import i3d_fold_bn_cases as C
from conftest import record_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K3, K3_BF = "mgar_conv3d_k3_fwd_affine", "mgar_conv3d_k3_bf16_fwd_affine"
STEM, STEM_BF = "mgar_stem_conv3d_fwd_affine", "mgar_stem_conv3d_bf16_fwd_affine"
AFFINE = (K3, K3_BF, STEM, STEM_BF)

ALL = [("k3", s, False) for s in C.K3_FP32] + [("k3", s, True) for s in C.K3_BF16] + [("stem", s, s[4]) for s in C.STEM]
IDS = ["%s-%s-%s" % (k, "x".join(str(int(v)) for v in s[:6 if k == "k3" else 4]), "bf16" if b else "fp32") for k, s, b in ALL]
FP32_CASES = [(c, i) for c, i in zip(ALL, IDS) if not c[2]]
BF16_CASES = [(c, i) for c, i in zip(ALL, IDS) if c[2]]


# ---- the entry points, called by name ---------------------------------------------------------------------------------------------
def _dt(bf16):
    return BF if bf16 else torch.float32


def run(kind, x, w, epilogue=None, y=None, bstride=None):
    """kind 'k3' / 'stem'; x a device tensor of the payload dtype, w fp32; epilogue None (the plain entry) or (scale, shift, relu)
    device tensors; y / bstride: a destination slice (k3 only)"""
    from multimodal_gar_amd import _lib as L
    bf16 = x.dtype == BF
    st = L.stream_of(x)
    if kind == "stem":
        n, _, t, h, wd = x.shape
        out = torch.empty((n, 64, (t + 1) // 2, (h + 1) // 2, (wd + 1) // 2), dtype=x.dtype, device=x.device)
        wp = torch.empty((L.raw("mgar_stem_conv3d_workspace_floats"),), dtype=torch.float32, device=x.device)
        if epilogue is None:
            L.payload_call("mgar_stem_conv3d_fwd", x.dtype, L.pptr(x, x.dtype), n, t, h, wd, L.fptr(w), L.fptr(wp), L.pptr(out, x.dtype), st)
        else:
            s, hh, relu = epilogue
            L.call(STEM_BF if bf16 else STEM, L.pptr(x, x.dtype), n, t, h, wd, L.fptr(w), L.fptr(wp), L.fptr(s), L.fptr(hh), int(relu),
                   L.pptr(out, x.dtype), st)
        return out
    n, cin, d, h, wd = x.shape
    cout = w.shape[0]
    out = torch.empty((n, cout, d, h, wd), dtype=x.dtype, device=x.device) if y is None else y
    if bf16:
        wp = torch.empty((L.raw("mgar_conv3d_k3_bf16_workspace_bytes", cin, cout),), dtype=torch.uint8, device=x.device)
    else:
        wp = torch.empty((L.raw("mgar_conv3d_k3_workspace_floats", cin, cout),), dtype=torch.float32, device=x.device)
    if epilogue is None:
        L.call("mgar_conv3d_k3_bf16_fwd" if bf16 else "mgar_conv3d_k3_fwd", L.pptr(x, x.dtype), n, cin, d, h, wd, L.fptr(w), cout,
               wp.data_ptr(), L.pptr(out, x.dtype), st)
    else:
        s, hh, relu = epilogue
        L.call(K3_BF if bf16 else K3, L.pptr(x, x.dtype), n, cin, d, h, wd, L.fptr(w), cout, wp.data_ptr(), L.fptr(s), L.fptr(hh),
               int(relu), out.data_ptr(), cout * d * h * wd if bstride is None else bstride, st)
    return out


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def device_case(kind, shape, bf16):
    """the case of i3d_fold_bn_cases with its operands on the device and the plain entry's output (computed once, shared)"""
    c = dict(C.k3_case(shape, bf16) if kind == "k3" else C.stem_case(shape))
    c["xg"], c["wg"] = c["x"].cuda().to(_dt(bf16)), c["w"].cuda()
    c["sg"], c["hg"] = torch.from_numpy(np.array(c["scale"])).cuda(), torch.from_numpy(np.array(c["shift"])).cuda()
    c["plain"] = run(kind, c["xg"], c["wg"])
    return c


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,bf16", ALL, ids=IDS)
def test_identity_epilogue_reproduces_the_plain_entry_bit_for_bit(kind, shape, bf16):
    c = device_case(kind, shape, bf16)
    cout = c["wg"].shape[0]
    one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
    got = run(kind, c["xg"], c["wg"], (one, zero, 0))
    assert same_bits(got, c["plain"])


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind,shape,bf16", [c for c, _ in FP32_CASES], ids=[i for _, i in FP32_CASES])
def test_fp32_epilogue_is_one_correctly_rounded_fma_of_the_plain_output(kind, shape, bf16, relu):
    """and stays inside the bound against the float64 convolution"""
    c = device_case(kind, shape, bf16)
    got = _np(run(kind, c["xg"], c["wg"], (c["sg"], c["hg"], relu)))
    v64 = C.reference(_np(c["plain"]), c["scale"], c["shift"], relu)
    used = float((np.abs(got - v64) / C.fma_bound(v64)).max())
    print("fma err / bound %.3f" % used)
    record_error("i3d affine fp32 %s fma err / bound" % kind, used, 1.0, 1.0)
    assert used <= 1.0, used
    if relu:
        assert not np.signbit(got[v64 <= 0]).any() and (got[v64 <= 0] == 0).all()      # a negative or -0 pre-activation gives +0
    truth = C.reference(c["z"], c["scale"], c["shift"], relu)
    used_t = float((np.abs(got - truth) / C.truth_bound_fp32(c["z"], c["scale"], c["shift"])).max())
    print("vs float64 convolution err / bound %.3f" % used_t)
    record_error("i3d affine fp32 %s vs fp64 conv err / bound" % kind, used_t, 1.0, 1.0)
    assert used_t <= 1.0, used_t


@pytest.mark.parametrize("kind,shape,bf16", [c for c, _ in BF16_CASES], ids=[i for _, i in BF16_CASES])
def test_bf16_epilogue_within_the_float64_bound_and_relu_is_a_clamp(kind, shape, bf16):
    c = device_case(kind, shape, bf16)
    outs = [run(kind, c["xg"], c["wg"], (c["sg"], c["hg"], relu)) for relu in (0, 1)]
    for relu, out in zip((0, 1), outs):
        assert out.dtype == BF
        ref = C.reference(c["z"], c["scale"], c["shift"], relu)
        used = float((np.abs(_np(out) - ref) / C.bound_bf16(c["z"], c["S"], c["n"], c["scale"], c["shift"], relu)).max())
        print("relu %d err / bound %.3f" % (relu, used))
        record_error("i3d affine bf16 %s relu=%d err / bound" % (kind, relu), used, 1.0, 1.0)
        assert used <= 1.0, (relu, used)
    # bf16 rounding is monotone and sign-preserving: out(relu = 1) = max(out(relu = 0), +0) bit for bit
    clamp = torch.where(outs[0] > 0, outs[0], torch.zeros_like(outs[0]))
    assert same_bits(outs[1], clamp)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 32, 3, 9, 20), (2, 8, 208, 2, 23, 160)], ids=["32ch", "208ch-tail"])
def test_k3_writes_a_channel_slice_and_nothing_else(shape, bf16):
    """N = 2, Y of Cout + 24 channels pre-filled with a sentinel, c0 = 8: the slice is the contiguous call's result bit for bit and
    every sentinel outside it is intact (second shape: the 64-channel groups and the 16-channel tail group are two launches)"""
    n, cin, cout, d, h, w = shape
    x, wt = C.k3_operands(shape, bf16)
    xg, wg = x.cuda().to(_dt(bf16)), wt.cuda()
    g = torch.Generator().manual_seed(3)
    ep = (torch.randn(cout, generator=g).cuda(), torch.randn(cout, generator=g).cuda(), 1)
    want = run("k3", xg, wg, ep)
    sentinel = -7.0
    Y = torch.full((n, cout + 24, d, h, w), sentinel, dtype=_dt(bf16), device="cuda")
    dst = Y[:, 8:8 + cout]
    run("k3", xg, wg, ep, y=dst, bstride=Y.stride(0))
    assert same_bits(dst, want)
    assert (Y[:, :8] == sentinel).all() and (Y[:, 8 + cout:] == sentinel).all()


@pytest.mark.parametrize("kind,shape,bf16", [("k3", C.K3_FP32[3], False), ("k3", C.K3_BF16[3], True), ("stem", C.STEM[1], False),
                                             ("stem", C.STEM[4], True)], ids=["k3-fp32", "k3-bf16", "stem-fp32", "stem-bf16"])
def test_repeatable_and_batch_independent(kind, shape, bf16):
    c = device_case(kind, shape, bf16)
    ep = (c["sg"], c["hg"], 1)
    a, b = run(kind, c["xg"], c["wg"], ep), run(kind, c["xg"], c["wg"], ep)
    assert same_bits(a, b)
    assert c["xg"].shape[0] > 1
    for n in range(c["xg"].shape[0]):
        one = run(kind, c["xg"][n:n + 1].contiguous(), c["wg"], ep)
        assert same_bits(one[0], a[n]), "sample %d of the batched launch differs from its N = 1 launch" % n
    assert run(kind, c["xg"][:0].contiguous(), c["wg"], ep).shape[0] == 0                   # N = 0: nothing launched


@pytest.mark.parametrize("kind,shape,bf16", [("k3", C.K3_FP32[1], False), ("k3", C.K3_BF16[1], True), ("stem", C.STEM[1], False),
                                             ("stem", C.STEM[2], False), ("stem", C.STEM[4], True)],
                         ids=["k3-fp32", "k3-bf16", "stem-minimal", "stem-direct", "stem-bf16"])
def test_one_nan_poisons_exactly_its_receptive_field_through_the_relu(kind, shape, bf16):
    """relu = 1: the NaN mask of the output is the float64 reference's (the receptive field of the poisoned element, every channel:
    the zero-scale channels too); every other element stays inside its bound"""
    c = device_case(kind, shape, bf16)
    x = c["x"].clone()
    pos = (0, 1, 1, 4, 5) if kind == "k3" else (0, 2, 1, 5, 6)
    x[pos] = float("nan")
    z, S = (C.k3_conv64 if kind == "k3" else C.stem_conv64)(x, c["w"])
    xg = x.cuda().to(_dt(bf16))
    got = _np(run(kind, xg, c["wg"], (c["sg"], c["hg"], 1)))
    mask = np.isnan(z)
    assert 0 < mask.sum() < mask.size and mask.any(axis=(0, 2, 3, 4)).all()                 # every channel, part of the volume
    if kind == "stem" and bf16:
        # the bf16 stem kernel pads the 7 taps of a row to the 8 k of an MFMA with a zero weight on input column 2 wo + 7: 0 x NaN
        # poisons one output column beyond the receptive field, in the plain entry as well.  The epilogue must add nothing to that.
        plain_mask = np.isnan(_np(run(kind, xg, c["wg"])))
        assert (plain_mask | ~mask).all() and 0 < plain_mask.sum() < mask.size
        mask = plain_mask
    assert np.array_equal(np.isnan(got), mask)
    ok = ~mask
    if bf16:
        zf, Sf = np.where(mask, 0.0, z), np.where(mask, 0.0, S)
        err = np.abs(got - C.reference(zf, c["scale"], c["shift"], 1)) / C.bound_bf16(zf, Sf, c["n"], c["scale"], c["shift"], 1)
    else:
        v64 = C.reference(_np(run(kind, xg, c["wg"])), c["scale"], c["shift"], 1)
        assert np.array_equal(np.isnan(v64), mask)
        err = np.abs(got - v64) / C.fma_bound(np.where(mask, 0.0, v64))
    assert float(err[ok].max()) <= 1.0


# ---- Unit3D -----------------------------------------------------------------------------------------------------------------------
def _record_calls(monkeypatch):
    from multimodal_gar_amd import _lib as L
    calls, inner = [], L.call

    def recording(name, *a):
        calls.append((name, a))
        return inner(name, *a)
    monkeypatch.setattr(L, "call", recording)
    return calls


def _units():
    from multimodal_gar_amd.model.backbone import Unit3D
    torch.manual_seed(5)
    k3 = Unit3D(32, 96, [3, 3, 3], name="k3")
    stem = Unit3D(3, 64, [7, 7, 7], stride=(2, 2, 2), padding=(3, 3, 3), name="stem")
    return [fill_deterministic(u, seed=4).cuda().eval() for u in (k3, stem)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_unit3d_eval_is_one_affine_call_and_the_old_route_otherwise(monkeypatch, bf16):
    from multimodal_gar_amd.model.backbone import Unit3D
    monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
    calls = _record_calls(monkeypatch)
    for u, x, want in zip(_units(), (torch.randn(2, 32, 3, 10, 12, device="cuda"), torch.randn(1, 3, 4, 12, 16, device="cuda")),
                          ((K3, K3_BF), (STEM, STEM_BF))):
        x = x.to(_dt(bf16))
        with torch.no_grad():
            del calls[:]
            fused = u(x)
            assert [c[0] for c in calls] == [want[bf16]], calls
            before = {k: v.clone() for k, v in u.bn.state_dict().items()}
            # the switch off: the convolution, then the BatchNorm kernel -- the route and the bits of calling the two halves directly
            monkeypatch.setattr(Unit3D, "fold_bn_eval", False)
            del calls[:]
            plain = u(x)
            names = [c[0] for c in calls]
            assert not set(names) & set(AFFINE) and any(n.startswith("mgar_bn_") for n in names), names
            assert names[0] in ("mgar_conv3d_k3_fwd", "mgar_conv3d_k3_bf16_fwd", "mgar_stem_conv3d_fwd", "mgar_stem_conv3d_fwd_bf16"), names
            del calls[:]
            halves = u._bn_relu(u._conv(x))
            assert [c[0] for c in calls] == names and same_bits(plain, halves)
            monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
            # train mode: batch statistics, the old route
            u.train()
            del calls[:]
            u(x)
            assert not set(c[0] for c in calls) & set(AFFINE)
            u.eval()
            u.bn.load_state_dict(before)                                 # (the train pass moved the running statistics)
        if not bf16:
            # a required gradient (grad mode on, parameters trainable): the old route (fp32: the library convolution takes no
            # bf16 input with an fp32 weight outside autocast)
            del calls[:]
            y = u(x)
            assert not set(c[0] for c in calls) & set(AFFINE) and y.requires_grad
        # fused and unfused agree.  fp32: the unfused kernel rounds ((z - m) invstd) gamma + beta four times, the fused route rounds
        # scale, shift and the fma -- at most 7 roundings of 2^-24 on terms |z s| + |m s| + |beta| <= about 2 x the output scale:
        # 14 * 2^-24 < 1e-6 of it, asserted with a factor 2.  bf16: both round once to bf16, one ulp = 2^-7 of the value apart.
        scale = plain.float().abs().max().item()
        err = (fused.float() - plain.float()).abs().max().item()
        record_error("Unit3D eval fused vs unfused", err, scale, 2.0 ** -7 if bf16 else 2e-6)
        assert err <= (2.0 ** -7 if bf16 else 2e-6) * scale, (err, scale)


# ---- InceptionModule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_inception_module_eval_writes_the_3x3x3_branches_into_the_concatenation(monkeypatch, bf16):
    from multimodal_gar_amd.model.backbone import InceptionModule, Unit3D
    monkeypatch.setattr(Unit3D, "fold_bn_eval", True)
    torch.manual_seed(2)
    oc = [64, 96, 128, 16, 32, 32]
    mod = fill_deterministic(InceptionModule(192, oc, "m"), seed=8).cuda().eval()
    if bf16:                                                            # bf16 payloads as the bf16 configurations run them
        for m in mod.modules():
            if isinstance(m, nn.Conv3d):
                m.weight.data = m.weight.data.to(BF)
    x = torch.relu(torch.randn(2, 192, 3, 9, 12, device="cuda")).to(_dt(bf16))
    calls = _record_calls(monkeypatch)
    copies = []
    inner_copy = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: copies.append(tuple(self.shape)) or inner_copy(self, *a, **k))
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=BF, enabled=bf16):
        y = mod(x)
        monkeypatch.setattr(torch.Tensor, "copy_", inner_copy)
        aff = [c for c in calls if c[0] in AFFINE]
        assert [c[0] for c in aff] == [K3_BF if bf16 else K3] * 2
        dhw, item = 3 * 9 * 12, y.element_size()
        total = oc[0] + oc[2] + oc[4] + oc[5]
        assert y.shape == (2, total, 3, 9, 12)
        for c, c0 in zip(aff, (oc[0], oc[0] + oc[2])):                 # destination: the branch's channels of y, y's batch stride
            assert c[1][12] == y.data_ptr() + c0 * dhw * item and c[1][13] == total * dhw
        assert copies == [], copies                                      # no branch needed the caller's copy
        monkeypatch.setattr(Unit3D, "fold_bn_eval", False)
        want = mod(x)
    scale = want.float().abs().max().item()
    err = (y.float() - want.float()).abs().max().item()
    record_error("InceptionModule eval fused vs unfused", err, scale, 2.0 ** -7 if bf16 else 1e-4)
    assert err <= (2.0 ** -7 if bf16 else 1e-4) * scale


# ---- the trunk ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunk():
    """(module on the device in eval mode with perturbed running statistics, x (2, 3, 5, 32, 64) on the device, float64 CPU result)"""
    from multimodal_gar_amd.model.backbone import InceptionI3d
    torch.manual_seed(21)
    net = InceptionI3d(final_endpoint="Mixed_4f")
    net.build()
    net = fill_deterministic(net, seed=6).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 3, 5, 32, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        truth = copy.deepcopy(net).double().extract_features(x.double())
    return net.cuda(), x.cuda(), truth


def _fold(monkeypatch, on):
    from multimodal_gar_amd.model.backbone import Unit3D
    monkeypatch.setattr(Unit3D, "fold_bn_eval", bool(on), raising=False)     # (absent before the fold existed: the several-clips tests still run there)


def test_trunk_eval_fused_is_as_close_to_float64_as_unfused(monkeypatch):
    net, x, truth = _trunk()
    calls = _record_calls(monkeypatch)
    outs = {}
    for on in (True, False):
        _fold(monkeypatch, on)
        del calls[:]
        with torch.no_grad():
            outs[on] = net.extract_features(x).double().cpu()
        names = [c[0] for c in calls]
        assert sum(n in AFFINE for n in names) == (16 if on else 0)
        outs[on, "bn"] = sum(n.startswith("mgar_bn_") for n in names)
    assert outs[True, "bn"] == outs[False, "bn"] - 16 and outs[True, "bn"] >= 29            # the 1x1x1 units keep their BatchNorm kernel
    scale = truth.abs().max().item()
    e_f, e_u = (outs[True] - truth).abs().max().item(), (outs[False] - truth).abs().max().item()
    print("trunk vs float64: fused %.3e unfused %.3e of the scale" % (e_f / scale, e_u / scale))
    record_error("I3D eval trunk fused vs fp64", e_f, scale, 1e-4)
    record_error("I3D eval trunk unfused vs fp64", e_u, scale, 1e-4)
    assert e_f <= 1e-4 * scale and e_u <= 1e-4 * scale
    assert e_f <= max(1.5 * e_u, 2e-6 * scale), (e_f, e_u, scale)


def test_trunk_eval_bf16_fused_is_no_farther_from_fp32_than_unfused(monkeypatch):
    net, x, _ = _trunk()
    net16 = copy.deepcopy(net)
    for m in net16.modules():
        if isinstance(m, nn.Conv3d):
            m.weight.data = m.weight.data.to(BF)
    outs = {}
    with torch.no_grad():
        _fold(monkeypatch, False)
        ref = net.extract_features(x).double()
        for on in (True, False):
            _fold(monkeypatch, on)
            with torch.autocast(device_type="cuda", dtype=BF):
                outs[on] = net16.extract_features(x)
            assert outs[on].dtype == BF
    norm = ref.pow(2).mean().sqrt().item()
    d_f, d_u = ((outs[on].double() - ref).pow(2).mean().sqrt().item() / norm for on in (True, False))
    print("bf16 eval trunk vs fp32, rel rms: fused %.3e, unfused %.3e" % (d_f, d_u))
    record_error("I3D eval bf16 trunk fused vs fp32 (rel rms)", d_f, 1.0, d_u)
    record_error("I3D eval bf16 trunk unfused vs fp32 (rel rms)", d_u, 1.0, d_u)
    assert d_f <= d_u, (d_f, d_u)


# ---- several clips in eval mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_i3d_eval_with_per_sample_stats_takes_two_clips(monkeypatch, fold):
    """per_sample_stats means nothing in eval mode (every clip sees the running statistics): two clips in one pass run, give the two
    one-clip results bit for bit, and leave every running buffer and num_batches_tracked alone -- fold switch on or off, 1x1x1
    units included."""
    net, x, _ = _trunk()
    _fold(monkeypatch, fold)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.set_per_sample_stats(True)
    try:
        with torch.no_grad():
            both = net.extract_features(x)
            singles = [net.extract_features(x[n:n + 1].contiguous()) for n in range(2)]
    finally:
        net.set_per_sample_stats(False)
    for n in range(2):
        assert same_bits(both[n], singles[n][0]), n
    after = net.state_dict()
    assert any(k.endswith("num_batches_tracked") for k in after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


def test_clip_model_eval_two_clips_gpu_vs_cpu_backend():
    """test_modules_gpu.test_clip_model_forward_gpu_vs_cpu_backend with two clips: on the device both go through I3D in one pass"""
    from multimodal_gar_amd import workload as W
    from oracle.cpu_backend import use_cpu_oracle
    torch.manual_seed(0)
    model = fill_deterministic(W.ClipModel(4, 1024), seed=11).eval()
    batch = W.make_batch(5, 2, 2, 4, 1024, 64, 96, torch.device("cpu"))
    with use_cpu_oracle(), torch.no_grad():
        want = model(batch)
    gm = copy.deepcopy(model).cuda()
    assert gm.batch_i3d
    before = {k: v.clone() for k, v in gm.state_dict().items()}
    gb = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    with torch.no_grad():
        got = gm(gb)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 16
    for a, b in zip(got, want):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        assert a.shape == b.shape
        scale = b.abs().max().item() + 1e-12
        err = (a - b).abs().max().item()
        record_error("ClipModel eval, two clips", err, scale, 1e-4)
        assert err <= 1e-5 + 1e-4 * scale, "max err %g vs scale %g" % (err, scale)
    after = gm.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
