"""csrc/pointwise_bf16.hip on the device: mgar_pointwise_mfma_bf16_fwd against the float64 reference of
tests/pointwise_bf16_cases.py on the ROUNDED operands (per-element bound: any fp32 accumulation order + one bf16 rounding), its
refusals, what it leaves untouched, position independence bit for bit, NaN propagation, the host routing in
multimodal_gar_amd/bn_ops.py, graph capture, and the drift of a bf16 shared MLP against its fp32 run."""
import copy

import pytest
import torch
import torch.nn as nn

import pointwise_bf16_cases as PC
from conftest import record_error

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NEW = "mgar_pointwise_mfma_bf16_fwd"
OLD = "mgar_pointwise_conv_fwd_bf16"
CANARY = -1.75                      # exactly representable in bf16
MGAR_EUNSUPPORTED = -3


def _d(t):
    return None if t is None else t.cuda()


def launch(x, w_store, strides, cout, mean=None, invstd=None, gamma=None, beta=None, relu=0, y=None, shape=None):
    """The entry point called by name on device tensors; ``shape`` overrides (B, Cin, P) for the refusal tests.  -> (rc, y)"""
    from multimodal_gar_amd import _lib as L
    b, cin, p = shape if shape is not None else x.shape
    if y is None:
        y = torch.full((b, cout, p), CANARY, dtype=BF, device="cuda")
    rc = L._fns[NEW](L.pptr(x, BF), b, cin, p, L.fptr(w_store), strides[0], strides[1], cout, L.fptr(mean), L.fptr(invstd),
                     L.fptr(gamma), L.fptr(beta), int(relu), L.pptr(y, BF), L.stream_of(x))
    return rc, y


def run_case(case, variant, x=None):
    ops = PC.operands(case, variant)
    x = _d(ops["x"]) if x is None else x
    rc, y = launch(x, _d(ops["w_store"]), ops["strides"], case[2], _d(ops["mean"]), _d(ops["invstd"]), _d(ops["gamma"]),
                   _d(ops["beta"]), ops["relu"])
    assert rc == 0
    return y


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", PC.VARIANTS)
@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_kernel_against_float64_on_the_rounded_operands(case, variant):
    ref, bound = PC.expected(case, variant)
    y = run_case(case, variant)
    assert y.dtype == BF and tuple(y.shape) == tuple(ref.shape)
    used = PC.share_of_bound(y.float().cpu(), ref, bound)
    what = "pointwise_bf16 %s %s" % (PC.case_id(case), variant)
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, what
    assert torch.equal(bits(y), bits(run_case(case, variant)))                      # two launches: identical bits


def test_refusals_write_nothing():
    from multimodal_gar_amd import _lib as L
    x = torch.randn(2, 260, 128, device="cuda").to(BF)
    w = torch.randn(70, 260, device="cuda")
    y = torch.full((2 * 70 * 128,), CANARY, dtype=BF, device="cuda")
    for cin, cout, p in ((16, 65, 128), (0, 16, 128), (257, 16, 128), (16, 16, 126)):
        rc, _ = launch(x, w, (max(cin, 1), 1), cout, y=y, shape=(2, cin, p))
        assert rc == MGAR_EUNSUPPORTED, (cin, cout, p, rc)
        assert "Cin" in L.raw("mgar_last_error").decode()
    for b, p in ((0, 128), (2, 0)):
        rc, _ = launch(x, w, (16, 1), 16, y=y, shape=(b, 16, p))
        assert rc == 0, (b, p, rc)
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())


@pytest.mark.parametrize("case", [c for c in PC.CASES if c[3] in (124, 132, 260)], ids=PC.case_id)
def test_nothing_outside_y_changes(case):
    """y sits inside a larger canary buffer (8-byte aligned, as the entry point requires): the ragged last tile of P = 124 / 132 /
    260 writes no element before or after it."""
    b, cin, cout, p, _ = case
    ops = PC.operands(case, "bn_relu")
    n, guard = b * cout * p, 1024
    buf = torch.full((n + 2 * guard,), CANARY, dtype=BF, device="cuda")
    y = buf[guard:guard + n].view(b, cout, p)
    rc, _ = launch(_d(ops["x"]), _d(ops["w_store"]), ops["strides"], cout, _d(ops["mean"]), _d(ops["invstd"]), _d(ops["gamma"]),
                   _d(ops["beta"]), 1, y=y)
    assert rc == 0
    assert bool((buf[:guard] == CANARY).all()) and bool((buf[guard + n:] == CANARY).all())
    assert torch.equal(bits(y), bits(run_case(case, "bn_relu")))


@pytest.mark.parametrize("variant", PC.VARIANTS)
def test_a_columns_bits_do_not_depend_on_its_position_or_on_the_launch(variant):
    case = PC.CASES[2]                                                              # (3, 35, 20, 4096)
    ops = PC.operands(case, variant)
    full = run_case(case, variant)
    x = _d(ops["x"])
    args = (_d(ops["w_store"]), ops["strides"], case[2], _d(ops["mean"]), _d(ops["invstd"]), _d(ops["gamma"]), _d(ops["beta"]),
            ops["relu"])
    rc, alone = launch(x[1:2].contiguous(), *args)                                  # sample 1 launched alone
    assert rc == 0 and torch.equal(bits(alone[0]), bits(full[1]))
    for s, p0 in ((0, 0), (2, 1152), (1, 3968)):                                    # 128 columns of a sample launched as P = 128
        rc, part = launch(x[s:s + 1, :, p0:p0 + 128].contiguous(), *args)
        assert rc == 0 and torch.equal(bits(part[0]), bits(full[s, :, p0:p0 + 128])), (s, p0)
    rc, part = launch(x[0:1, :, 4:12].contiguous(), *args)                          # another offset inside the tile, P = 8
    assert rc == 0 and torch.equal(bits(part[0]), bits(full[0, :, 4:12]))


@pytest.mark.parametrize("case,where", [(PC.CASES[2], (1, 34, 4095)), (PC.CASES[2], (0, 0, 130)), (PC.CASES[5], (1, 255, 259)),
                                        (PC.CASES[3], (1, 16, 129))], ids=lambda v: PC.case_id(v) if len(v) == 5 else "%d_%d_%d" % v)
def test_one_nan_makes_its_column_nan_and_no_other(case, where):
    ref, bound = PC.expected(case, "bn_relu")
    x = _d(PC.operands(case, "bn_relu")["x"]).clone()
    b, i, p = where
    x[b, i, p] = float("nan")
    y = run_case(case, "bn_relu", x=x).float().cpu()
    assert bool(torch.isnan(y[b, :, p]).all())
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[b, :, p] = False
    assert bool(torch.isfinite(y[keep]).all())
    err = (y.double() - ref).abs()
    assert bool((err[keep] <= bound[keep]).all())


# ---- the host routing -----------------------------------------------------------------------------------------------------------
class _CallLog:
    """Names of the library entry points reached while it is active (the calls go through)."""

    def __init__(self, monkeypatch):
        from multimodal_gar_amd import _lib as L
        self.names = []
        inner = L.call

        def call(name, *args):
            self.names.append(name)
            return inner(name, *args)
        monkeypatch.setattr(L, "call", call)


def _mlp(spec, seed):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import shared_mlp_2d
    torch.manual_seed(seed)
    net = shared_mlp_2d(list(spec))
    for m in net:
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.8, 1.2)
            nn.init.uniform_(m.bias, -0.2, 0.2)
    return net.cuda().train()


def test_routing(monkeypatch):
    from multimodal_gar_amd import _lib as L, bn_ops
    net = _mlp((16, 16, 32), seed=3)
    torch.manual_seed(4)
    x = torch.randn(2, 16, 1024, 32, device="cuda").to(BF)
    log = _CallLog(monkeypatch)

    def run(inp, module=net, grad=False):
        del log.names[:]
        m = copy.deepcopy(module)                                                   # every run from the same running statistics
        with torch.set_grad_enabled(grad):
            out = m(inp)
        torch.cuda.synchronize()
        return out, list(log.names)

    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", True)
    out, names = run(x)
    assert names.count(NEW) == 2 and OLD not in names, names                        # the first conv (no prologue) and the hidden step
    # the same chain spelled out: direct calls of the entry point, the module's own statistics and final BatchNorm + ReLU
    ref = copy.deepcopy(net)
    w1, w2 = ref[0].weight.detach().view(16, 16), ref[3].weight.detach().view(32, 16)
    x3 = x.flatten(2)
    rc, y1 = launch(x3, w1, (16, 1), 16)
    assert rc == 0
    mean, invstd = bn_ops._train_stats(y1, ref[1])
    rc, y2 = launch(y1, w2, (16, 1), 32, mean, invstd, ref[1].weight.detach(), ref[1].bias.detach(), 1)
    assert rc == 0
    with torch.no_grad():
        want = bn_ops.bn_act(y2.view(2, 32, 1024, 32), ref[4], True)
    assert out.dtype == BF and torch.equal(bits(out), bits(want))

    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", False)
    off, names = run(x)
    assert names.count(OLD) == 2 and NEW not in names, names
    fns = dict(L._fns)
    del fns[NEW]
    monkeypatch.setattr(L, "_fns", fns)                                             # the symbol is gone: the route must not miss it
    off2, names = run(x)
    assert names.count(OLD) == 2 and torch.equal(bits(off), bits(off2))
    monkeypatch.undo()

    log = _CallLog(monkeypatch)
    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", True)
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", True)
    _, names = run(x.float())                                                      # fp32 payload
    assert NEW not in names and OLD not in names and any(n.startswith("mgar_pointwise_conv_fwd") for n in names), names
    _, names = run(x, module=copy.deepcopy(net).eval())                             # eval mode: the inference route, untouched
    assert NEW not in names and names.count(OLD) == 2, names
    # a required gradient: bf16 is a forward path, the fused steps refuse as before and never reach the new symbol
    m = copy.deepcopy(net)
    xg = x.clone().requires_grad_(True)
    del log.names[:]
    assert bn_ops.plain_conv(xg, m[0], bf16_mfma=True) is None and bn_ops.plain_conv(x, m[0], bf16_mfma=True) is None
    assert bn_ops.bn_act_conv(xg, m[1], True, m[3]) is None and bn_ops.bn_act_conv(x, m[1], True, m[3]) is None
    assert NEW not in log.names and OLD not in log.names
    for q in m[0].parameters():
        q.requires_grad_(False)
    for q in m[3].parameters():
        q.requires_grad_(False)
    y = bn_ops.bn_act_conv(x, m[1], True, m[3])                                     # the BatchNorm's affine alone wants one
    assert y is not None and y.dtype == BF and NEW not in log.names and log.names.count(OLD) == 1, log.names
    with torch.no_grad():
        del log.names[:]
        assert bn_ops.plain_conv(x, m[0]) is not None and log.names == [OLD]        # consent withheld (the default)
        del log.names[:]
        assert bn_ops.plain_conv(x, m[0], bf16_mfma=True) is not None and log.names == [NEW]

def test_graph_capture_replays_the_eager_bits():
    case = PC.CASES[6]                                                              # (3, 32, 64, 644)
    ops = PC.operands(case, "bn_relu")
    eager = run_case(case, "bn_relu")
    x = _d(ops["x"])
    args = (_d(ops["w_store"]), ops["strides"], case[2], _d(ops["mean"]), _d(ops["invstd"]), _d(ops["gamma"]), _d(ops["beta"]), 1)
    y = torch.full(tuple(eager.shape), CANARY, dtype=BF, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        launch(x, *args, y=y)                                                       # warm-up on the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            rc, _ = launch(x, *args, y=y)
        assert rc == 0
    for _ in range(2):
        y.fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(eager))


# ---- module drift ---------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def _conv_fp32(x4, w):
    """conv 1x1 on the existing fp32 entry point, no prologue"""
    from multimodal_gar_amd import _lib as L
    b, c = x4.shape[:2]
    x3 = x4.contiguous().flatten(2)
    cout, p = w.shape[0], x3.shape[2]
    w = w.contiguous()
    y = torch.empty((b, cout, p), device="cuda")
    L.call("mgar_pointwise_conv_fwd", L.fptr(x3), b, c, p, L.fptr(w), c, 1, cout, None, None, None, None, 0, L.fptr(y), L.stream_of(x3))
    return y.view(b, cout, *x4.shape[2:])


def _emulation(net, x):
    """The bf16 route restated on the existing fp32 entry points alone, rounded to bf16 where the bf16 route rounds: every weight,
    every conv output, every activated conv input, the pooled output.  The two differ in summation order alone."""
    from multimodal_gar_amd import bn_ops

    def r(t):
        return t.to(BF).float()
    layers = list(copy.deepcopy(net))
    convs = [m for m in layers if isinstance(m, nn.Conv2d)]
    bns = [m for m in layers if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        h = r(_conv_fp32(x.float(), r(convs[0].weight.view(convs[0].out_channels, -1))))
        for conv, bn in zip(convs[1:], bns[:-1]):
            a = r(bn_ops.bn_act(h, bn, True))                                       # mgar_bn_train_stats + mgar_bn_act_fwd, fp32
            h = r(_conv_fp32(a, r(conv.weight.view(conv.out_channels, -1))))
        return r(bn_ops.bn_act_maxpool(h, bns[-1], True))                           # mgar_bn_act_maxpool_fwd, fp32


@pytest.mark.parametrize("spec,m,ns", [((4, 16, 16, 32), 2048, 16), ((4, 32, 32, 64), 1024, 32)], ids=["sa1_ns16", "sa1_ns32"])
def test_module_drift_against_fp32(spec, m, ns, monkeypatch):
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", True)
    net = _mlp(spec, seed=7)
    torch.manual_seed(8)
    x = torch.randn(2, spec[0], m, ns, device="cuda").to(BF)
    assert x.shape[0] * m * ns == 65536
    log = _CallLog(monkeypatch)
    with torch.no_grad():
        out32 = copy.deepcopy(net).forward_maxpool(x.float())
        del log.names[:]
        out16 = copy.deepcopy(net).forward_maxpool(x)
        assert log.names.count(NEW) == 3 and OLD not in log.names, log.names
        emu = _emulation(net, x)
    assert out16.dtype == BF and out32.dtype == torch.float32 and out16.shape == out32.shape == emu.shape
    d_own, d_emu = _rel_rms(out16.float(), out32), _rel_rms(emu, out32)
    tol = max(1.5 * d_emu, 1e-3)
    print("shared MLP %s ns %d: bf16 vs fp32 rel rms %.3e, emulation on the fp32 kernels %.3e" % (spec, ns, d_own, d_emu))
    record_error("shared MLP %s bf16 vs fp32 (rel rms)" % (spec,), d_own, 1.0, tol)
    record_error("shared MLP %s emulation vs fp32 (rel rms)" % (spec,), d_emu, 1.0, tol)
    assert d_emu > 0
    assert d_own <= tol, (d_own, d_emu)
