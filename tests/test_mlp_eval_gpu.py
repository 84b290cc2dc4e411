"""Device tests of the inference shared-MLP route: the kernel (mgar_pointwise_conv_maxpool_eval_fwd /
mgar_pointwise_conv_maxpool_eval_bf16_fwd, csrc/pointwise_fwd.hip MAXPOOL epilogue) against the float64 reference and
per-element bound of mlp_eval_cases.py, bit equality with max(dim=-1) of mgar_pointwise_conv_fwd under an identity epilogue,
repeatability, position independence, NaN / inf behaviour, refusals; then the host route: PointwiseSequential.forward_maxpool
fused against switch-off against a float64 truth, which entry points each mode reaches, and graph capture.

Measured on an MI355X (max err / bound over all cases): fp32 0.384, bf16 0.994; see test_values' docstring."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_eval_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP32, BF16 = "mgar_pointwise_conv_maxpool_eval_fwd", "mgar_pointwise_conv_maxpool_eval_bf16_fwd"
MGAR_OK, MGAR_EUNSUPPORTED = 0, -3
CASE_IDS = [E.case_id(c) for c in E.CASES]
SMALL_IDS = [E.case_id(c) for c in E.SMALL_CASES]


def _L():
    from multimodal_gar_amd import _lib as L
    return L


def _cuda(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).cuda()               # a copy: the shared cases are read-only
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=4)
def _device_case(case, bf16):
    d = E.make_case(case, bf16)
    out = {k: _cuda(d[k]) for k in ("mean", "invstd", "gamma", "beta", "w", "scale", "shift")}
    out["x"] = _cuda(d["x"], BF if bf16 else torch.float32)
    out["in_relu"], out["out_relu"] = d["in_relu"], d["out_relu"]
    return out


def _pool(d, x=None, scale=None, shift=None, out_relu=None, raw=False):
    """-> the flat (B * Cout * M + PAD_OUT) buffer, pre-filled with the sentinel; the kernel writes its first B * Cout * M"""
    L = _L()
    x = d["x"] if x is None else x
    scale = d["scale"] if scale is None else scale
    shift = d["shift"] if shift is None else shift
    out_relu = d["out_relu"] if out_relu is None else out_relu
    b, cin, m, ns = x.shape
    cout = d["w"].shape[0]
    buf = torch.full((b * cout * m + E.PAD_OUT,), E.SENTINEL, dtype=x.dtype, device="cuda")
    args = (L.pptr(x, x.dtype), b, cin, m, ns, L.fptr(d["w"]), cin, 1, cout, L.fptr(d["mean"]), L.fptr(d["invstd"]), L.fptr(d["gamma"]),
            L.fptr(d["beta"]), d["in_relu"], L.fptr(scale), L.fptr(shift), out_relu, buf.data_ptr(), L.stream_of(x))
    name = FP32 if x.dtype == torch.float32 else BF16
    rc = L.raw(name, *args) if raw else L.call(name, *args)
    torch.cuda.synchronize()
    return (rc, buf) if raw else buf


def _body(buf, b, cout, m):
    return buf[:b * cout * m].view(b, cout, m)


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", E.CASES, ids=CASE_IDS)
def test_values(case, bf16):
    """Every case x payload inside the bound of mlp_eval_cases.py; the elements behind the pooled tensor keep their sentinel bit
    for bit; with out_relu every value is >= 0 and none is -0.
    Measured max err / bound on an MI355X, worst over the 33 cases: fp32 0.384 (B1_1to64_M5_ns64_id_r00), bf16 0.994
    (B1_4to4_M32801_ns32_bn_r11; the bf16 bound is one rounding at 2^-8 and is attained next to a power of two)."""
    (b, _, cout, m, _), _, _, out_relu = case
    d = _device_case(case, bf16)
    buf = _pool(d)
    assert buf.dtype == (BF if bf16 else torch.float32)
    assert (buf[b * cout * m:] == E.SENTINEL).all(), "elements beyond the pooled tensor were written"
    got = _body(buf, b, cout, m).double().cpu().numpy()
    assert np.isfinite(got).all()
    u = E.used(got, case, bf16)
    print("%s %s: max err / bound = %.3f" % (E.case_id(case), "bf16" if bf16 else "fp32", u))
    assert u <= 1.0, u
    if out_relu:
        assert (got >= 0).all() and not np.signbit(got).any()


# ---- bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", E.CASES, ids=CASE_IDS)
def test_bit_anchor_identity_epilogue(case, bf16):
    """scale = 1, shift = 0, no output ReLU: torch.equal to max(dim=-1) of mgar_pointwise_conv_fwd's output on the same operands
    (the kernel the existing op-level tests carry; bf16: rounding is monotone, so rounding before or after the max agrees)."""
    L = _L()
    (b, cin, cout, m, ns), _, _, _ = case
    d = _device_case(case, bf16)
    x, dt = d["x"], d["x"].dtype
    one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
    got = _body(_pool(d, scale=one, shift=zero, out_relu=0), b, cout, m)
    y = torch.empty((b, cout, m, ns), dtype=dt, device="cuda")
    L.payload_call("mgar_pointwise_conv_fwd", dt, L.pptr(x, dt), b, cin, m * ns, L.fptr(d["w"]), cin, 1, cout, L.fptr(d["mean"]),
                   L.fptr(d["invstd"]), L.fptr(d["gamma"]), L.fptr(d["beta"]), d["in_relu"], L.pptr(y, dt), L.stream_of(x))
    torch.cuda.synchronize()
    yf = y.float()
    assert torch.isfinite(yf).all() and not ((yf == 0) & torch.signbit(yf)).any()      # no -0 for fmaf(z, 1, +0) to normalise
    assert torch.equal(got, y.max(dim=-1).values)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", E.WIDTH_CASES, ids=[E.case_id(c) for c in E.WIDTH_CASES])
def test_bit_repeatable_and_position_independent(case, bf16):
    """The same launch twice gives the same bits; the second sample in a launch of its own (B = 1: other tiles, other waves)
    gives the bits of that sample."""
    (b, _, cout, m, _), _, _, _ = case
    d = _device_case(case, bf16)
    first, again = _pool(d), _pool(d)
    assert torch.equal(first, again)
    sub = _pool(d, x=d["x"][1:].contiguous())
    assert (sub[cout * m:] == E.SENTINEL).all()
    assert torch.equal(_body(sub, 1, cout, m), _body(first, b, cout, m)[1:])


# ---- NaN and inf ------------------------------------------------------------------------------------------------------------------
_ID_CASES = [c for c in E.WIDTH_CASES if c[1] == "id"]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", _ID_CASES, ids=[E.case_id(c) for c in _ID_CASES])
def test_nan_and_inf_stay_in_their_groups(case, bf16):
    """Identity prologue (a = x): a NaN in one column makes every output channel of its group NaN; a +inf (-inf) column makes
    channel o of its group +inf where W[o, c] scale_o > 0 (< 0) and leaves a finite value elsewhere; every other group keeps its
    bits."""
    (b, cin, cout, m, ns), _, _, _ = case
    d = _device_case(case, bf16)
    clean = _body(_pool(d), b, cout, m)
    x = d["x"].clone()
    c = cin - 1
    spots = {"nan": (0, 0, ns - 1), "+inf": (1, m - 1, 1), "-inf": (1, 0, ns // 2)}       # (sample, group, slot), last channel
    x[0, 0, 0, ns - 1] = float("nan")
    x[1, c, m - 1, 1] = float("inf")
    x[1, c, 0, ns // 2] = float("-inf")
    got = _body(_pool(d, x=x), b, cout, m)
    assert torch.isnan(got[0, :, 0]).all()
    sign = torch.sign(d["w"][:, c] * d["scale"])
    assert (sign != 0).all()
    for name, s in (("+inf", 1.0), ("-inf", -1.0)):
        bb, mm, _ = spots[name]
        col = got[bb, :, mm].float()
        assert not torch.isnan(col).any(), name
        assert (col[sign * s > 0] == float("inf")).all(), name
        assert torch.isfinite(col[sign * s < 0]).all(), name
    keep = torch.ones((b, m), dtype=torch.bool, device="cuda")
    for bb, mm, _ in spots.values():
        keep[bb, mm] = False
    keep = keep[:, None, :].expand(b, cout, m)
    assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_nan_through_both_relus(bf16):
    """BatchNorm + ReLU prologue, ReLU epilogue (relu_nan on both sides): the NaN group is NaN in every channel, nothing else moves."""
    case = next(c for c in E.WIDTH_CASES if c[1] == "bn" and c[2] and c[3] and c[0][4] == 64)
    (b, cin, cout, m, ns), _, _, _ = case
    d = _device_case(case, bf16)
    clean = _body(_pool(d), b, cout, m)
    x = d["x"].clone()
    x[1, cin // 2, m - 1, ns - 3] = float("nan")
    got = _body(_pool(d, x=x), b, cout, m)
    assert torch.isnan(got[1, :, m - 1]).all()
    keep = torch.ones((b, cout, m), dtype=torch.bool, device="cuda")
    keep[1, :, m - 1] = False
    assert torch.equal(got[keep], clean[keep])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_unsupported_and_empty(bf16):
    L = _L()
    dt = BF if bf16 else torch.float32

    def run(b, cin, cout, m, ns):
        d = {"x": torch.ones((b, cin, m, ns), dtype=dt, device="cuda"), "w": torch.ones((cout, cin), device="cuda"),
             "scale": torch.ones(max(cout, 1), device="cuda"), "shift": torch.ones(max(cout, 1), device="cuda"),
             "mean": None, "invstd": None, "gamma": None, "beta": None, "in_relu": 0, "out_relu": 0}
        return _pool(d, raw=True)

    for shape in ((1, 8, 8, 4, 24), (1, 8, 65, 4, 16), (1, 8, 8, 4, 6), (1, 8, 8, 4, 1), (1, 8, 8, 2, 256)):
        rc, buf = run(*shape)
        assert rc == MGAR_EUNSUPPORTED, shape
        assert b"pointwise_conv_maxpool_eval" in L._fns["mgar_last_error"]()
        assert (buf == E.SENTINEL).all(), shape
    for shape in ((0, 8, 8, 4, 16), (2, 8, 8, 0, 16)):
        rc, buf = run(*shape)
        assert rc == MGAR_OK and (buf == E.SENTINEL).all(), shape


# ---- the host route -------------------------------------------------------------------------------------------------------------
SPECS = {"6_16_16_32": ([6, 16, 16, 32], (2, 2048, 16)), "35_32_32_64": ([35, 32, 32, 64], (1, 2048, 32))}


def _mlp(spec):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import shared_mlp_2d
    return fill_deterministic(shared_mlp_2d(list(spec)), seed=3).eval()


@functools.lru_cache(maxsize=None)
def _host_case(key, start, bf16):
    """-> (module on the device, input of forward_maxpool(start=start) on the device, truth float64 (B, C', M) on the CPU,
    bf16 bounds {fused: , unfused: } or None).  start = 1: the input is the first conv's output, as "project, then group" hands it
    over; the truth starts from that same tensor."""
    spec, (b, m, ns) = SPECS[key]
    mod = _mlp(spec)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((b, spec[0], m, ns), generator=g)
    ref = copy.deepcopy(mod).double()
    with torch.no_grad():
        if start == 1:
            x = torch.einsum("oi,bims->boms", mod[0].weight.view(spec[1], spec[0]), x)
        if bf16:
            x = x.to(BF)
        x64 = x.double()
        truth = ref[start:](x64).max(dim=3).values
        bounds = _bf16_chain_bounds(ref, start, x64) if bf16 else None
    return mod.cuda(), x.cuda(), truth, bounds


def _bf16_chain_bounds(ref, start, x64):
    """Per-element bounds of the bf16 routes against the float64 chain on the same bf16 input, with the rounding term of
    mlp_eval_cases.py (2^-8 (|value| + E) per stored bf16 tensor) carried through the layers: a conv maps E to |W| E, an eval
    BatchNorm to |scale| E, ReLU and max are 1-Lipschitz; the fp32 arithmetic in between adds gamma(Cin + 8) |W| |a|.
    fused: every hidden conv output is stored once, the pooled tensor once.  unfused: every conv output AND every activated
    tensor is stored, the pooled tensor once.  -> {True: (B, C', M), False: (B, C', M)}"""
    import torch_refs as R
    out = {}
    for fused in (True, False):
        v, e = x64, torch.zeros_like(x64)
        layers = list(ref)[start:]
        for k, layer in enumerate(layers):
            if isinstance(layer, nn.Conv2d):
                w = layer.weight.view(layer.out_channels, layer.in_channels)
                z = torch.einsum("oi,bims->boms", w, v)
                e = torch.einsum("oi,bims->boms", w.abs(), e + R.gamma_u(layer.in_channels + 8) * v.abs())
                last = not any(isinstance(t, nn.Conv2d) for t in layers[k + 1:])
                if not (fused and last):
                    e = e + E.BF16_EPS * (z.abs() + e)                      # the conv output is stored in bf16
                v = z
            elif isinstance(layer, nn.BatchNorm2d):
                sc = (layer.weight / torch.sqrt(layer.running_var + layer.eps)).view(1, -1, 1, 1)
                v = layer(v)
                e = sc.abs() * e + 8 * E.U * v.abs()
            else:
                v = torch.relu(v)
                if not fused and k + 1 < len(layers):
                    e = e + E.BF16_EPS * (v.abs() + e)                      # the activated tensor is stored in bf16
        pooled, e = v.max(dim=3).values, e.max(dim=3).values
        out[fused] = e + E.BF16_EPS * (pooled.abs() + e)
    return out


def _forward(mod, x, start, autocast=False):
    with torch.autocast("cuda", dtype=BF, enabled=autocast):
        y = mod.forward_maxpool(x, start=start)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("key", sorted(SPECS))
def test_module_fused_against_switch_off_against_float64(key, start, bf16, monkeypatch):
    """PointwiseSequential as the SA modules build it, .eval() with non-trivial running statistics, through forward_maxpool.
    fp32: both routes within 1e-4 max |truth|; bf16 under autocast: each route within its per-element bound
    (_bf16_chain_bounds); either payload: the fused error is not above twice the switch-off error.
    Measured on an MI355X, fused / switch-off: fp32 1.1e-6 .. 1.4e-6 / 1.1e-6 .. 1.6e-6 at max |truth| 5.2 .. 6.7; bf16 2.2e-2 ..
    3.1e-2 / 3.4e-2 .. 4.7e-2, max err / bound 0.17 .. 0.56 / 0.16 .. 0.32."""
    from multimodal_gar_amd import bn_ops
    mod, x, truth, bounds = _host_case(key, start, bf16)
    runs = {}
    for fuse in (True, False):
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", fuse)
        with torch.no_grad():
            runs[fuse] = _forward(mod, x, start, autocast=bf16)
        assert runs[fuse].shape == truth.shape and runs[fuse].dtype == (BF if bf16 else torch.float32)
    scale = truth.abs().max().item()
    err = {fuse: (runs[fuse].double().cpu() - truth).abs() for fuse in (True, False)}
    worst = {fuse: err[fuse].max().item() for fuse in (True, False)}
    print("%s start %d %s: fused err %.3e, unfused err %.3e, max |truth| %.3e" % (key, start, "bf16" if bf16 else "fp32", worst[True],
                                                                                   worst[False], scale))
    if bf16:
        for fuse in (True, False):
            u = (err[fuse] / bounds[fuse]).max().item()
            print("    %s: max err / bound = %.3f" % ("fused" if fuse else "unfused", u))
            assert u <= 1.0, (fuse, u)
    else:
        assert worst[True] <= 1e-4 * scale and worst[False] <= 1e-4 * scale
    assert worst[True] <= 2.0 * worst[False]


# ---- routing --------------------------------------------------------------------------------------------------------------------
def _census(monkeypatch, fn):
    """entry points of the library reached while fn() runs -> ({name: calls}, fn's result)"""
    L = _L()
    calls, inner = {}, L.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    monkeypatch.setattr(L, "call", counting)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(L, "call", inner)
    return calls, out


def _parent_route(mod, x, start):
    """What forward_maxpool ran in eval mode before the inference route existed, spelled out: the streaming kernel for a leading
    conv it takes (else the library GEMM), bn_act + library GEMM for every hidden layer, bn_act_maxpool at the end."""
    from multimodal_gar_amd import bn_ops, nn_utils
    layers = list(mod)[start:]
    i = 0
    while i < len(layers):
        layer = layers[i]
        if isinstance(layer, nn.Conv2d):
            y = bn_ops.plain_conv(x, layer)
            x = y if y is not None else nn_utils.conv1x1(layer, x)
            i += 1
        else:
            assert isinstance(layer, nn.BatchNorm2d) and isinstance(layers[i + 1], nn.ReLU)
            x = bn_ops.bn_act_maxpool(x, layer, True) if i + 2 >= len(layers) else bn_ops.bn_act(x, layer, True)
            i += 2
    return x


@pytest.mark.parametrize("key", sorted(SPECS))
def test_routing(key, monkeypatch):
    """Eval + no_grad: the tail is one call of the new entry, the hidden layer one mgar_pointwise_conv_fwd, and no mgar_bn_act*
    entry runs.  The switch off, train mode, a required gradient and ns = 24 each reach exactly the entries they reach with the
    route disabled -- never the new one -- with equal bits; the switch-off output has the bits of the parent's route."""
    from multimodal_gar_amd import bn_ops
    spec, (b, m, ns) = SPECS[key]
    mod, x, _, _ = _host_case(key, 0, False)
    new = (FP32, BF16)

    def bn_entries(calls):
        return sum(n for k, n in calls.items() if k.startswith("mgar_bn_act"))

    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    with torch.no_grad():
        calls, _ = _census(monkeypatch, lambda: _forward(mod, x, 0))
        assert calls.get(FP32) == 1 and calls.get(BF16) is None and bn_entries(calls) == 0, calls
        assert calls.get("mgar_pointwise_conv_fwd") == (2 if spec[0] <= 32 else 1), calls
        calls, out = _census(monkeypatch, lambda: _forward(mod, x.to(BF), 0, autocast=True))
        assert calls.get(BF16) == 1 and calls.get(FP32) is None and bn_entries(calls) == 0 and out.dtype == BF, calls
        calls, _ = _census(monkeypatch, lambda: _forward(mod, _host_case(key, 1, False)[1], 1))
        assert calls.get(FP32) == 1 and calls.get("mgar_pointwise_conv_fwd") == 1 and bn_entries(calls) == 0, calls
        # an MLP whose only conv is its first layer: the identity-prologue form
        single = fill_deterministic(type(mod)(*copy.deepcopy(list(mod)[:3])), seed=5).eval().cuda()
        calls, out = _census(monkeypatch, lambda: _forward(single, x, 0))
        assert calls == {FP32: 1} and out.shape == (b, spec[1], m), calls

    def both(make, run):
        """run(module) with the route enabled and disabled, on fresh copies -> census of either run; asserts equal bits"""
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
        calls_on, on = _census(monkeypatch, lambda: run(make()))
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", False)
        calls_off, off = _census(monkeypatch, lambda: run(make()))
        monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
        assert torch.equal(on, off) and calls_on == calls_off, (calls_on, calls_off)
        assert not any(k in new for k in calls_on)
        return calls_on

    def no_grad(mod_):
        with torch.no_grad():
            return _forward(mod_, x, 0)
    calls = both(lambda: copy.deepcopy(mod).train(), no_grad)                                   # train mode
    assert calls.get("mgar_bn_act_maxpool_fwd") == 1, calls
    both(lambda: copy.deepcopy(mod), lambda mod_: _forward(mod_, x, 0).detach())               # eval, the parameters want a gradient
    # ns = 24, outside the epilogue's group widths: the whole MLP, hidden steps included, keeps today's route
    x24 = torch.randn((b, spec[0], m * ns // 16, 24), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        calls = both(lambda: mod, lambda mod_: _forward(mod_, x24, 0))
    assert calls.get("mgar_bn_act_maxpool_fwd") == 1 and calls.get("mgar_bn_act_fwd") == 2, calls
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", False)                                         # the switch
    with torch.no_grad():
        calls, off = _census(monkeypatch, lambda: _forward(mod, x, 0))
        assert not any(k in new for k in calls) and calls.get("mgar_bn_act_maxpool_fwd") == 1 and calls.get("mgar_bn_act_fwd") == 2, calls
        assert torch.equal(off, _parent_route(mod, x, 0))


def test_hook_keeps_the_old_route(monkeypatch):
    from multimodal_gar_amd import bn_ops
    mod, x, _, _ = _host_case("6_16_16_32", 0, False)
    hooked = copy.deepcopy(mod)
    seen = []
    hooked[6].register_forward_hook(lambda m, i, o: seen.append(1))
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    with torch.no_grad():
        calls, _ = _census(monkeypatch, lambda: _forward(hooked, x, 0))
    assert FP32 not in calls and calls.get("mgar_bn_act_maxpool_fwd") == 1, calls


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits(monkeypatch):
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    mod, x, _, _ = _host_case("35_32_32_64", 0, False)
    with torch.no_grad():
        eager = _forward(mod, x, 0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod.forward_maxpool(x)                       # warm-up on the capture's side stream: fold_bn cached, allocator primed
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mod.forward_maxpool(x)
        out.fill_(E.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
