"""csrc/pointwise_wide_bf16.hip on the device: mgar_pointwise_wide_bf16_fwd / mgar_pointwise_wide_maxpool_bf16_fwd against the
float64 reference of tests/pointwise_wide_bf16_cases.py on the ROUNDED operands (per-element bounds: any fp32 accumulation order,
the one fma of the affine store, one bf16 rounding), their refusals, what they leave untouched, position independence bit for
bit, NaN / inf propagation, the I3D entry points of the same kernel (mgar_conv1x1_bf16_fwd[_affine]) as the same contract bit
for bit on their own timer row, the host routing in multimodal_gar_amd/bn_ops.py, nn_utils.py and the FP module with a call
census, graph capture, and the drift of bf16 shared MLPs against their fp32 run (train mode) and the float64 chain (eval mode).

Measured on an MI355X: largest err / bound over the 81 unpooled case x prologue x store combinations 0.993 (the bound is the
store rounding's: 2^-8 |ref| dominates), over the five pooled cases 0.976."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import pointwise_wide_bf16_cases as WC
from conftest import record_error

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FWD, POOL = "mgar_pointwise_wide_bf16_fwd", "mgar_pointwise_wide_maxpool_bf16_fwd"
NARROW = "mgar_pointwise_mfma_bf16_fwd"
CANARY = -1.75                      # exactly representable in bf16
MGAR_OK, MGAR_EUNSUPPORTED = 0, -3
U, BF16_EPS = 2.0 ** -24, 2.0 ** -8


def _L():
    from multimodal_gar_amd import _lib as L
    return L


def _d(t):
    if t is None:
        return None
    return (torch.from_numpy(np.array(t)) if isinstance(t, np.ndarray) else t).cuda()


def bits(t):
    return t.contiguous().view(torch.int16)


def launch(x, w_full, w_off, w_ld, cout, pro=None, scale=None, shift=None, out_relu=0, y=None, shape=None, ybs=None, ns=0):
    """An entry point called by name on device tensors.  w_full: the stored weight, W[0, 0] lies w_off floats behind its start;
    pro = (mean, invstd, gamma, beta, relu) | None; ns: the pooled entry, x (B, Cin, M * ns); ``shape`` overrides (B, Cin, P)
    -- pooled: (B, Cin, M) -- for the refusal tests.  -> (rc, y)"""
    L = _L()
    b, cin, p = shape if shape is not None else ((x.shape[0], x.shape[1], x.shape[2] // ns) if ns else x.shape)
    mean, invstd, gamma, beta, relu = pro if pro is not None else (None, None, None, None, 0)
    if y is None:
        y = torch.full((b, cout, p), CANARY, dtype=BF, device="cuda")
    wp = w_full.data_ptr() + 4 * w_off
    if ns:
        rc = L._fns[POOL](L.pptr(x, BF), b, cin, p, ns, wp, w_ld, cout, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                          int(relu), L.fptr(scale), L.fptr(shift), int(out_relu), y.data_ptr(), L.stream_of(x))
    else:
        rc = L._fns[FWD](L.pptr(x, BF), b, cin, p, wp, w_ld, cout, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                         int(relu), L.fptr(scale), L.fptr(shift), int(out_relu), y.data_ptr(),
                         cout * p if ybs is None else ybs, L.stream_of(x))
    return rc, y


def _pro(ops):
    return None if ops["mean"] is None else (_d(ops["mean"]), _d(ops["invstd"]), _d(ops["gamma"]), _d(ops["beta"]), ops["relu"])


def run_case(case, prologue, store, x=None, **kw):
    ops = WC.operands(case, prologue)
    scale, shift, relu = WC.store_args(case, prologue, store)
    x = _d(ops["x"]) if x is None else x
    rc, y = launch(x, _d(ops["w_full"]), ops["w_off"], ops["w_ld"], case[2], _pro(ops), _d(scale), _d(shift), relu, **kw)
    assert rc == 0
    return y


def run_pooled(pc, x=None):
    (b, cin, cout, m, ns), prologue, orl = pc
    ops = WC.operands(WC.pooled_as_case(pc), prologue)
    e = WC.pooled_expected(pc)
    x = _d(ops["x"]) if x is None else x
    rc, y = launch(x, _d(ops["w_full"]), 0, cin, cout, _pro(ops), _d(e["scale"]), _d(e["shift"]), orl, ns=ns)
    assert rc == 0
    return y


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", WC.STORES)
@pytest.mark.parametrize("prologue", WC.PROLOGUES)
@pytest.mark.parametrize("case", WC.CASES, ids=WC.case_id)
def test_kernel_against_float64_on_the_rounded_operands(case, prologue, store):
    ref, bound = WC.store_expected(case, prologue, store)
    y = run_case(case, prologue, store)
    assert y.dtype == BF and tuple(y.shape) == tuple(ref.shape)
    used = WC.share(y.float().cpu().numpy(), ref, bound)
    what = "pointwise_wide_bf16 %s %s %s" % (WC.case_id(case), prologue, store)
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, what
    assert torch.equal(bits(y), bits(run_case(case, prologue, store)))                  # two launches: identical bits


@pytest.mark.parametrize("pc", WC.POOLED, ids=WC.pooled_id)
def test_pooled_kernel_against_float64_on_the_rounded_operands(pc):
    e = WC.pooled_expected(pc)
    y = run_pooled(pc)
    assert y.dtype == BF and tuple(y.shape) == tuple(e["ref"].shape)
    used = WC.share(y.float().cpu().numpy(), e["ref"], e["bound"])
    what = "pointwise_wide_maxpool_bf16 %s" % WC.pooled_id(pc)
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, what
    assert torch.equal(bits(y), bits(run_pooled(pc)))


# ---- one contract with the I3D entry points -------------------------------------------------------------------------------------
def _conv1x1(x, w, cout, scale=None, shift=None, relu=0, y=None, ybs=None):
    """mgar_conv1x1_bf16_fwd, or with a scale mgar_conv1x1_bf16_fwd_affine, called by name -> (rc, y)"""
    L = _L()
    n, cin, p = x.shape
    if y is None:
        y = torch.full((n, cout, p), CANARY, dtype=BF, device="cuda")
    ybs = cout * p if ybs is None else ybs
    if scale is None:
        rc = L._fns["mgar_conv1x1_bf16_fwd"](L.pptr(x, BF), n, cin, p, L.fptr(w), cout, y.data_ptr(), ybs, L.stream_of(x))
    else:
        rc = L._fns["mgar_conv1x1_bf16_fwd_affine"](L.pptr(x, BF), n, cin, p, L.fptr(w), cout, L.fptr(scale), L.fptr(shift), int(relu),
                                                    y.data_ptr(), ybs, L.stream_of(x))
    return rc, y


@pytest.mark.parametrize("cin,cout,gap", [(20, 24, 0), (40, 40, 0), (72, 96, 64), (136, 160, 0), (520, 264, 0)],
                         ids=lambda v: str(v))
def test_conv1x1_entries_and_the_wide_entry_are_one_contract(cin, cout, gap):
    """The same x, w and scale / shift through mgar_conv1x1_bf16_fwd[_affine] and through mgar_pointwise_wide_bf16_fwd with the
    identity prologue and w_ld = Cin: identical bits, each call on its own timer row.  One case per Cout tier, ragged channels,
    P = 132 = a full tile and a 4-column tail; (520, 264) has W in several chunks and 8 waves; ``gap``: y_batch_stride beyond
    Cout * P, the padding untouched."""
    L = _L()
    n, p = 2, 132
    g = torch.Generator().manual_seed(1000 * cin + cout)
    x = torch.randn((n, cin, p), generator=g).to(BF).cuda()
    w = (torch.randn((cout, cin), generator=g) / cin ** 0.5).cuda()
    scale = (torch.rand((cout,), generator=g) * 2.0 - 0.5).cuda()                       # both signs
    shift = torch.randn((cout,), generator=g).cuda()
    ybs = cout * p + gap

    def timed(fn):
        """-> (y (n, ybs) with its padding, the timer rows the call added to)"""
        y = torch.full((n, ybs), CANARY, dtype=BF, device="cuda")
        L.kernel_timers()                                                               # reset
        rc, _ = fn(y)
        assert rc == MGAR_OK
        rows = L.kernel_timers()
        assert bool((y[:, cout * p:] == CANARY).all())
        return y, rows

    was_on = L._KT_STATE["on"]
    L.kernel_timers(enable=True)
    try:
        for sc, sh, relu in ((None, None, 0), (scale, shift, 0), (scale, shift, 1)):
            y1, rows1 = timed(lambda y: _conv1x1(x, w, cout, sc, sh, relu, y=y, ybs=ybs))
            y2, rows2 = timed(lambda y: launch(x, w, 0, cin, cout, None, sc, sh, relu, y=y, ybs=ybs))
            assert torch.equal(bits(y1), bits(y2)), (sc is not None, relu)
            assert not bool((y1[:, :cout * p] == CANARY).all())
            assert set(rows1) == {"conv1x1_bf16_kernel"} and set(rows2) == {"pointwise_wide_bf16_kernel"}, (rows1, rows2)
            work = (1, 2.0 * n * p * (cin + cout), 2.0 * n * p * cin * cout)            # launches, bytes, flop
            assert rows1["conv1x1_bf16_kernel"][1:] == work and rows2["pointwise_wide_bf16_kernel"][1:] == work
    finally:
        L.kernel_timers(enable=was_on)


def test_refusals_write_nothing():
    L = _L()
    x = torch.randn(2, 1030, 128, device="cuda").to(BF)
    w = torch.randn(520, 1030, device="cuda")
    v = torch.ones(1030, device="cuda")
    y = torch.full((2 * 520 * 128,), CANARY, dtype=BF, device="cuda")
    #                     Cin, Cout,   P, w_ld
    for cin, cout, p, ld in ((0, 16, 128, 16), (1025, 16, 128, 1030), (128, 513, 128, 128), (128, 128, 126, 128), (128, 128, 128, 127)):
        for pro in (None, (v, v, v, v, 1)):
            rc, _ = launch(x, w, 0, ld, cout, pro, v, v, 1, y=y, shape=(2, cin, p))
            assert rc == MGAR_EUNSUPPORTED, (cin, cout, p, ld, rc)
            assert b"pointwise_wide_bf16_fwd" in L._fns["mgar_last_error"]()
    #                     Cin, Cout, M, ns, w_ld
    for cin, cout, m, ns, ld in ((128, 128, 4, 24, 128), (0, 16, 4, 16, 16), (1025, 16, 4, 16, 1030), (128, 513, 4, 16, 128),
                                 (128, 128, 4, 16, 127), (128, 128, 42, 3, 128)):
        rc, _ = launch(x, w, 0, ld, cout, None, v, v, 1, y=y, shape=(2, cin, m), ns=ns)
        assert rc == MGAR_EUNSUPPORTED, (cin, cout, m, ns, ld, rc)
        assert b"pointwise_wide_maxpool_bf16_fwd" in L._fns["mgar_last_error"]()
    for b, p in ((0, 128), (2, 0)):                                                     # empty shapes
        rc, _ = launch(x, w, 0, 128, 128, None, y=y, shape=(b, 128, p))
        assert rc == MGAR_OK, (b, p, rc)
        rc, _ = launch(x, w, 0, 128, 128, None, v, v, 1, y=y, shape=(b, 128, p), ns=16)
        assert rc == MGAR_OK, (b, p, rc)
    torch.cuda.synchronize()
    assert bool((y == CANARY).all())


@pytest.mark.parametrize("store", ["plain", "affine_relu"])
@pytest.mark.parametrize("case", [c for c in WC.CASES if c[3] in (132, 516, 644, 260, 8)], ids=WC.case_id)
def test_nothing_outside_y_changes(case, store):
    """y sits inside a larger canary buffer, its samples a gap apart (y_batch_stride = Cout * P + 64): the ragged tiles and row
    blocks write no element before, between or after the samples."""
    b, cin, cout, p, _ = case
    n, guard, gap = cout * p, 1024, 64
    buf = torch.full((guard + b * (n + gap) + guard,), CANARY, dtype=BF, device="cuda")
    y = buf[guard:guard + b * (n + gap)].view(b, n + gap)
    run_case(case, "bn_relu", store, y=y, ybs=n + gap)
    dense = run_case(case, "bn_relu", store)
    assert bool((buf[:guard] == CANARY).all()) and bool((buf[guard + b * (n + gap):] == CANARY).all())
    assert bool((y[:, n:] == CANARY).all())
    assert torch.equal(bits(y[:, :n]), bits(dense.view(b, n)))


@pytest.mark.parametrize("pc", [WC.POOLED[1], WC.POOLED[3]], ids=WC.pooled_id)
def test_nothing_outside_the_pooled_y_changes(pc):
    (b, cin, cout, m, ns), _, _ = pc
    n, guard = b * cout * m, 1024
    pad = (-n) % 4                                                                      # y 8-byte aligned
    buf = torch.full((guard + n + pad + guard,), CANARY, dtype=BF, device="cuda")
    y = buf[guard:guard + n].view(b, cout, m)
    ops = WC.operands(WC.pooled_as_case(pc), pc[1])
    e = WC.pooled_expected(pc)
    rc, _ = launch(_d(ops["x"]), _d(ops["w_full"]), 0, cin, cout, _pro(ops), _d(e["scale"]), _d(e["shift"]), pc[2], y=y, ns=ns)
    assert rc == 0
    assert bool((buf[:guard] == CANARY).all()) and bool((buf[guard + n:] == CANARY).all())
    assert torch.equal(bits(y), bits(run_pooled(pc)))


@pytest.mark.parametrize("store", ["plain", "affine_relu"])
@pytest.mark.parametrize("prologue", WC.PROLOGUES)
def test_a_columns_bits_do_not_depend_on_its_position_or_on_the_launch(prologue, store):
    case = WC.CASES[5]                                                                  # (3, 196, 256, 644)
    full = run_case(case, prologue, store)
    x = _d(WC.operands(case, prologue)["x"])
    alone = run_case(case, prologue, store, x=x[1:2].contiguous())                        # sample 1 launched alone
    assert torch.equal(bits(alone[0]), bits(full[1]))
    for s, p0 in ((0, 0), (2, 384), (1, 516)):                                          # 128 columns launched as P = 128
        part = run_case(case, prologue, store, x=x[s:s + 1, :, p0:p0 + 128].contiguous())
        assert torch.equal(bits(part[0]), bits(full[s, :, p0:p0 + 128])), (s, p0)
    part = run_case(case, prologue, store, x=x[0:1, :, 4:12].contiguous())              # another offset inside a tile, P = 8
    assert torch.equal(bits(part[0]), bits(full[0, :, 4:12]))


@pytest.mark.parametrize("pc", [WC.POOLED[1], WC.POOLED[2]], ids=WC.pooled_id)
def test_a_groups_bits_do_not_depend_on_its_position(pc):
    (b, cin, cout, m, ns), prologue, orl = pc
    full = run_pooled(pc)
    ops = WC.operands(WC.pooled_as_case(pc), prologue)
    e = WC.pooled_expected(pc)
    x = _d(ops["x"])
    for s, g in ((0, 0), (b - 1, m - 1), (1, 5)):                                       # one group launched alone
        rc, one = launch(x[s:s + 1, :, g * ns:(g + 1) * ns].contiguous(), _d(ops["w_full"]), 0, cin, cout, _pro(ops), _d(e["scale"]),
                         _d(e["shift"]), orl, ns=ns)
        assert rc == 0 and torch.equal(bits(one[0, :, 0]), bits(full[s, :, g])), (s, g)


@pytest.mark.parametrize("case,where", [(WC.CASES[5], (1, 195, 643)), (WC.CASES[5], (0, 0, 130)), (WC.CASES[6], (1, 1023, 259)),
                                        (WC.CASES[1], (1, 16, 129))], ids=lambda v: WC.case_id(v) if len(v) == 5 else "%d_%d_%d" % v)
def test_one_nan_makes_its_column_nan_and_no_other(case, where):
    """through both ReLUs: the BatchNorm + ReLU prologue and the affine + ReLU store"""
    ref, bound = WC.store_expected(case, "bn_relu", "affine_relu")
    x = _d(WC.operands(case, "bn_relu")["x"]).clone()
    b, i, p = where
    x[b, i, p] = float("nan")
    y = run_case(case, "bn_relu", "affine_relu", x=x).float().cpu().numpy()
    assert np.isnan(y[b, :, p]).all()
    keep = np.ones(ref.shape, bool)
    keep[b, :, p] = False
    assert np.isfinite(y[keep]).all()
    assert (np.abs(y.astype(np.float64) - ref)[keep] <= bound[keep]).all()


@pytest.mark.parametrize("pc", [WC.POOLED[0], WC.POOLED[1], WC.POOLED[4]], ids=WC.pooled_id)
def test_pooled_nan_and_inf_stay_in_their_group(pc):
    (b, cin, cout, m, ns), prologue, orl = pc
    assert orl == 1
    clean = run_pooled(pc)
    x0 = _d(WC.operands(WC.pooled_as_case(pc), prologue)["x"])
    s, g = b - 1, m - 2
    keep = torch.ones((b, cout, m), dtype=torch.bool, device="cuda")
    keep[s, :, g] = False
    for slot in (0, ns - 3):                                                            # the group's first lane and a later one
        x = x0.clone()
        x[s, cin // 2, g * ns + slot] = float("nan")
        got = run_pooled(pc, x=x)
        assert bool(torch.isnan(got[s, :, g]).all()), slot                              # every channel of the group, zero scale included
        assert torch.equal(bits(got)[keep], bits(clean)[keep]), slot
    for v in (float("inf"), float("-inf")):
        x = x0.clone()
        x[s, cin // 2, g * ns + 1] = v
        got = run_pooled(pc, x=x)
        assert torch.equal(bits(got)[keep], bits(clean)[keep])


# ---- graph capture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [False, True], ids=["unpooled", "pooled"])
def test_graph_capture_replays_the_eager_bits(pooled):
    if pooled:
        pc = WC.POOLED[2]
        (b, cin, cout, m, ns), prologue, orl = pc
        ops, e = WC.operands(WC.pooled_as_case(pc), prologue), WC.pooled_expected(pc)
        eager = run_pooled(pc)
        args = (_d(ops["x"]), _d(ops["w_full"]), 0, cin, cout, _pro(ops), _d(e["scale"]), _d(e["shift"]), orl)
        kw = {"ns": ns}
    else:
        case = WC.CASES[6]           # (2, 1024, 512, 260): more than 64 KB of LDS, whose limit is raised at every launch -- captured ones too
        ops = WC.operands(case, "bn_relu")
        scale, shift, relu = WC.store_args(case, "bn_relu", "affine_relu")
        eager = run_case(case, "bn_relu", "affine_relu")
        args = (_d(ops["x"]), _d(ops["w_full"]), ops["w_off"], ops["w_ld"], case[2], _pro(ops), _d(scale), _d(shift), relu)
        kw = {}
    y = torch.full(tuple(eager.shape), CANARY, dtype=BF, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        launch(*args, y=y, **kw)                                                        # warm-up on the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            rc, _ = launch(*args, y=y, **kw)
        assert rc == 0
    for _ in range(2):
        y.fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(eager))


# ---- the host routing -----------------------------------------------------------------------------------------------------------
class _CallLog:
    """Names of the library entry points reached while it is active (the calls go through)."""

    def __init__(self, monkeypatch):
        L = _L()
        self.names = []
        inner = L.call

        def call(name, *args):
            self.names.append(name)
            return inner(name, *args)
        monkeypatch.setattr(L, "call", call)


def _mlp(spec, seed=3):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import shared_mlp_2d
    return fill_deterministic(shared_mlp_2d(list(spec)), seed=seed).cuda().train()


def _run(log, fn, grad=False, autocast=True):
    """fn() under bf16 autocast (today's route reaches the library GEMM with an fp32 weight; an fp32 payload runs without it: the
    first GEMM would hand bf16 on) -> (output, names reached)"""
    del log.names[:]
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=BF, enabled=autocast):
        out = fn()
    torch.cuda.synchronize()
    return out, list(log.names)


def _wide(names):
    return [n for n in names if n in (FWD, POOL)]


def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def _on(monkeypatch, wide=True, fuse=True, lift=True):
    """the switches; ``lift``: the plan's own gates (128 / 128, set by measurement) lifted to the kernel's limits, so that the
    routes are exercised at every width the kernel takes"""
    from multimodal_gar_amd import bn_ops
    monkeypatch.setattr(bn_ops, "MLP_BF16_WIDE", wide)
    monkeypatch.setattr(bn_ops, "WIDE_PLAN_MAX_IN", bn_ops.WIDE_MAX_IN if lift else 128)
    monkeypatch.setattr(bn_ops, "WIDE_PLAN_MAX_OUT", bn_ops.WIDE_MAX_OUT if lift else 128)
    monkeypatch.setattr(bn_ops, "MLP_EVAL_FUSE", fuse)
    monkeypatch.setattr(bn_ops, "MLP_BF16_MFMA", True)


def test_routing_of_a_train_mode_mlp(monkeypatch):
    """(128, 128, 256) through forward(): the first conv (identity prologue) and the hidden step (batch statistics in the
    prologue) are one launch each; the result is the chain of direct calls bit for bit."""
    from multimodal_gar_amd import bn_ops
    net = _mlp((128, 128, 256))
    torch.manual_seed(4)
    x = torch.randn(2, 128, 1024, 32, device="cuda").to(BF)
    log = _CallLog(monkeypatch)
    _on(monkeypatch)
    out, names = _run(log, lambda: copy.deepcopy(net)(x))
    assert names.count(FWD) == 2 and POOL not in names, names
    n_bn = sum(n.startswith("mgar_bn_act") for n in names)                              # the final BatchNorm + ReLU alone
    ref = copy.deepcopy(net)
    w1, w2 = ref[0].weight.detach().view(128, 128).contiguous(), ref[3].weight.detach().view(256, 128).contiguous()
    with torch.no_grad():
        rc, y1 = launch(x.flatten(2), w1, 0, 128, 128)
        assert rc == 0
        mean, invstd = bn_ops._train_stats(y1, ref[1])
        rc, y2 = launch(y1, w2, 0, 128, 256, (mean, invstd, ref[1].weight.detach(), ref[1].bias.detach(), 1))
        assert rc == 0
        want = bn_ops.bn_act(y2.view(2, 256, 1024, 32), ref[4], True)
    assert out.dtype == BF and torch.equal(bits(out), bits(want))
    _on(monkeypatch, lift=False)                                                        # the plan's own gates: 128 -> 256 stays
    _, names = _run(log, lambda: copy.deepcopy(net)(x))
    assert names.count(FWD) == 1 and sum(n.startswith("mgar_bn_act") for n in names) == n_bn + 1, names
    _on(monkeypatch)
    # each of these reaches exactly today's entries with today's bits: the switch off is today's route
    _on(monkeypatch, wide=False)
    off, names_off = _run(log, lambda: copy.deepcopy(net)(x))
    assert not _wide(names_off) and sum(n.startswith("mgar_bn_act") for n in names_off) == n_bn + 1, names_off
    _on(monkeypatch)
    L = _L()
    fns = dict(L._fns)
    del fns[FWD], fns[POOL]
    monkeypatch.setattr(L, "_fns", fns)                                                 # a library without the symbols
    nosym, names = _run(log, lambda: copy.deepcopy(net)(x))
    assert names == names_off and torch.equal(bits(nosym), bits(off))
    monkeypatch.undo()

    log = _CallLog(monkeypatch)

    def both(fn, grad=False, autocast=True):
        _on(monkeypatch, wide=False)
        a = _run(log, fn, grad, autocast)
        _on(monkeypatch, wide=True)
        b = _run(log, fn, grad, autocast)
        return a, b
    (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(net)(x.float()), autocast=False)   # an fp32 payload
    assert not _wide(n_on) and n_on == n_off and torch.equal(o_on, o_off)
    xg = x.clone().requires_grad_(True)                                                 # a required gradient
    (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(net)(xg), grad=True)
    assert not _wide(n_on) and n_on == n_off and torch.equal(bits(o_on.detach()), bits(o_off.detach()))
    (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(net)(x), grad=True)       # ... by the parameters alone
    assert not _wide(n_on) and n_on == n_off and torch.equal(bits(o_on.detach()), bits(o_off.detach()))
    hooked = copy.deepcopy(net)
    hooked[3].register_forward_hook(lambda *a: None)                                    # a forward hook on the hidden conv
    (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(hooked)(x))
    assert n_on.count(FWD) == 1 and not _wide(n_off), n_on                              # the first conv still goes
    hooked[0].register_forward_hook(lambda *a: None)
    (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(hooked)(x))
    assert not _wide(n_on) and n_on == n_off and torch.equal(bits(o_on), bits(o_off))
    narrow = _mlp((16, 16, 32))                                                         # a narrow MLP never reaches the new symbols
    xn = torch.randn(2, 16, 1024, 32, device="cuda").to(BF)
    for mod in (narrow, copy.deepcopy(narrow).eval()):
        (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(mod)(xn))
        assert not _wide(n_on) and n_on == n_off and torch.equal(bits(o_on), bits(o_off))
        (o_off, n_off), (o_on, n_on) = both(lambda: copy.deepcopy(mod).forward_maxpool(xn))
        assert not _wide(n_on) and n_on == n_off and torch.equal(bits(o_on), bits(o_off))


@pytest.mark.parametrize("lift", [False, True], ids=["shipped_gates", "lifted_gates"])
def test_routing_of_an_sa_level_2_mlp(lift, monkeypatch):
    """(99, 64, 64, 128) through forward_maxpool(start=1), as "project, then group" hands it over.  Train mode: the 64 -> 64 step
    stays on the narrow kernel, the 64 -> 128 step is one wide launch, the tail stays on bn_act_maxpool.  Eval mode: the tail
    [BN -> ReLU -> conv -> BN -> ReLU -> max] is ONE pooled launch and no mgar_bn_act* call is left."""
    from multimodal_gar_amd import bn_ops
    from multimodal_gar_amd.sparse_ops import fold_bn
    net = _mlp((99, 64, 64, 128))
    torch.manual_seed(5)
    x = torch.randn(2, 64, 1024, 32, device="cuda").to(BF)
    log = _CallLog(monkeypatch)
    _on(monkeypatch, lift=lift)
    out, names = _run(log, lambda: copy.deepcopy(net).forward_maxpool(x, start=1))
    assert names.count(FWD) == 1 and names.count(NARROW) == 1 and POOL not in names, names
    assert any(n.startswith("mgar_bn_act_maxpool_fwd") for n in names), names
    assert out.dtype == BF and tuple(out.shape) == (2, 128, 1024)
    _on(monkeypatch, lift=lift, wide=False)
    off, names_off = _run(log, lambda: copy.deepcopy(net).forward_maxpool(x, start=1))
    assert not _wide(names_off)
    d = _rel_rms(out.float(), off.float())
    print("SA level 2 train: wide vs today's route rel rms %.3e" % d)
    assert d < 2e-2                                                                     # two bf16 routes of the same chain

    ev = copy.deepcopy(net).eval()
    _on(monkeypatch, lift=lift)
    out, names = _run(log, lambda: ev.forward_maxpool(x, start=1))
    assert names.count(POOL) == 1 and FWD not in names and not any(n.startswith("mgar_bn_act") for n in names), names
    # the same chain spelled out: the narrow eval step as the module runs it, then one direct pooled call
    with torch.no_grad():
        h = bn_ops.bn_act_conv(x, ev[1], True, ev[3], others=(ev[2],))
        assert h is not None
        mean, invstd = bn_ops._stats(h.flatten(2), ev[4])
        scale, shift = fold_bn(ev[7])
        rc, want = launch(h.flatten(2), ev[6].weight.detach().view(128, 64).contiguous(), 0, 64, 128,
                          (mean, invstd, ev[4].weight.detach(), ev[4].bias.detach(), 1), scale, shift, 1, ns=32)
    assert rc == 0 and torch.equal(bits(out), bits(want))
    for kw in ({"wide": False}, {"fuse": False}):                                       # either switch off: today's calls
        _on(monkeypatch, lift=lift, **kw)
        off, names_off = _run(log, lambda: ev.forward_maxpool(x, start=1))
        assert not _wide(names_off), (kw, names_off)
        assert _rel_rms(out.float(), off.float()) < 2e-2
    _on(monkeypatch, lift=lift, wide=False, fuse=False)
    base, names_base = _run(log, lambda: ev.forward_maxpool(x, start=1))
    _on(monkeypatch, lift=lift, wide=True, fuse=False)
    off, names_off = _run(log, lambda: ev.forward_maxpool(x, start=1))
    assert names_off == names_base and torch.equal(bits(off), bits(base))               # MLP_EVAL_FUSE=0: bit for bit
    # ns = 24: the whole eval-mode MLP keeps today's route
    x24 = torch.randn(2, 64, 1366, 24, device="cuda").to(BF)
    _on(monkeypatch, lift=lift, wide=False)
    base, names_base = _run(log, lambda: ev.forward_maxpool(x24, start=1))
    _on(monkeypatch, lift=lift)
    got, names = _run(log, lambda: ev.forward_maxpool(x24, start=1))
    assert not _wide(names) and names == names_base and torch.equal(bits(got), bits(base))
    # a forward hook on the last BatchNorm: no pooled launch; the hidden step may still go
    hooked = copy.deepcopy(ev)
    hooked[7].register_forward_hook(lambda *a: None)
    got, names = _run(log, lambda: hooked.forward_maxpool(x, start=1))
    assert POOL not in names and names.count(FWD) == 1, names


@pytest.mark.parametrize("lift", [False, True], ids=["shipped_gates", "lifted_gates"])
def test_routing_of_an_fp_module(lift, monkeypatch):
    """PointnetFPModule [128 + 64 -> 128 -> 128]: both projections are one launch each on the weight's column slices; train mode
    adds the hidden step, eval mode the affine tail [BN -> ReLU -> conv -> BN -> ReLU] as one launch with no mgar_bn_act* left."""
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import PointnetFPModule
    torch.manual_seed(6)
    fp = PointnetFPModule(mlp=[192, 128, 128])
    fill_deterministic(fp, seed=5)
    fp = fp.cuda().train()
    b, n, m = 2, 32768, 32768
    known_feats = torch.randn(b, 128, m, device="cuda").to(BF)
    skip = torch.randn(b, 64, n, device="cuda").to(BF)
    idx = torch.randint(0, m, (b, n, 3), device="cuda", dtype=torch.int32)
    wgt = torch.rand(b, n, 3, device="cuda") + 0.1
    wgt = wgt / wgt.sum(dim=2, keepdim=True)
    xyz = torch.zeros(b, 1, 3, device="cuda")
    log = _CallLog(monkeypatch)

    def fwd(mod):
        return lambda: copy.deepcopy(mod)(xyz, xyz, skip, known_feats, nn_weights=(idx, wgt))
    for mod, eval_mode in ((fp, False), (copy.deepcopy(fp).eval(), True)):
        _on(monkeypatch, lift=lift)
        out, names = _run(log, fwd(mod))
        assert names.count(FWD) == 3 and POOL not in names, names
        if eval_mode:
            assert not any(n.startswith("mgar_bn_act") for n in names), names
        assert out.dtype == BF and tuple(out.shape) == (b, 128, n)
        _on(monkeypatch, lift=lift, wide=False)
        off, names_off = _run(log, fwd(mod))
        assert not _wide(names_off), names_off
        d = _rel_rms(out.float(), off.float())
        print("FP module %s: wide vs today's route rel rms %.3e" % ("eval" if eval_mode else "train", d))
        assert d < 2e-2
        _on(monkeypatch, lift=lift, wide=True)
        (o32, n32) = _run(log, lambda: copy.deepcopy(mod)(xyz, xyz, skip.float(), known_feats.float(), nn_weights=(idx, wgt)),
                          autocast=False)
        assert not _wide(n32), n32                                                      # fp32 payloads stay
    # the projections alone, against direct calls on the column slices
    from multimodal_gar_amd import bn_ops
    _on(monkeypatch, lift=lift)
    with torch.no_grad():
        conv = fp.mlp[0]
        zf = bn_ops.conv_bf16_wide(known_feats, conv, cols=(0, 128))
        zs = bn_ops.conv_bf16_wide(skip, conv, cols=(128, 192))
        w = conv.weight.detach().view(128, 192).contiguous()
        rc, wf = launch(known_feats, w, 0, 192, 128)
        rc2, ws = launch(skip, w, 128, 192, 128)
    assert rc == 0 and rc2 == 0 and torch.equal(bits(zf), bits(wf)) and torch.equal(bits(zs), bits(ws))
    # an x whose address is not 8-byte aligned goes back to the caller's route (the entry point would refuse it)
    flat = torch.zeros(skip.numel() + 4, dtype=BF, device="cuda")
    with torch.no_grad():
        for off, taken in ((0, True), (1, False), (2, False), (4, True)):
            view = flat[off:off + skip.numel()].view(skip.shape)
            assert view.is_contiguous() and (view.data_ptr() % 8 == 0) == taken
            assert (bn_ops.conv_bf16_wide(view, conv, cols=(128, 192)) is not None) == taken, off
    ref = torch.einsum("oi,bip->bop", w[:, 128:].to(BF).double(), skip.double())
    assert (zs.double() - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()


# ---- module drift ---------------------------------------------------------------------------------------------------------------
def _emulation(net, x, start):
    """The bf16 route restated in fp32 on today's fp32 route (library GEMM, mgar_bn_train_stats + mgar_bn_act_fwd,
    mgar_bn_act_maxpool_fwd), rounded to bf16 where the bf16 route rounds: every weight, every conv output, every activated conv
    input, the pooled output.  The two differ in summation order alone."""
    from multimodal_gar_amd import bn_ops

    def r(t):
        return t.to(BF).float()

    def conv(h, m):
        return r(torch.einsum("oi,bims->boms", r(m.weight.view(m.out_channels, -1)), h))
    layers = list(copy.deepcopy(net))[start:]
    convs = [m for m in layers if isinstance(m, nn.Conv2d)]
    bns = [m for m in layers if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        h = x.float()
        if isinstance(layers[0], nn.Conv2d):
            h = conv(h, convs.pop(0))
        for c, bn in zip(convs, bns[:-1]):
            h = conv(r(bn_ops.bn_act(h, bn, True)), c)
        return r(bn_ops.bn_act_maxpool(h, bns[-1], True))


@pytest.mark.parametrize("spec,start,cin", [((99, 64, 64, 128), 1, 64), ((128, 128, 128, 256), 0, 128)], ids=["sa2", "sa3"])
def test_train_mode_drift_against_fp32(spec, start, cin, monkeypatch):
    """Measured on an MI355X, bf16 against fp32 / emulation against fp32, relative RMS: (99, 64, 64, 128) from layer 1
    3.525e-3 / 3.525e-3, (128, 128, 128, 256) 3.903e-3 / 3.903e-3 -- the kernel and the emulation agree to the printed digits."""
    _on(monkeypatch)
    net = _mlp(spec, seed=7)
    torch.manual_seed(8)
    x = torch.randn(2, cin, 1024, 32, device="cuda").to(BF)
    log = _CallLog(monkeypatch)
    with torch.no_grad():
        out32 = copy.deepcopy(net).forward_maxpool(x.float(), start=start)
        out16, names = _run(log, lambda: copy.deepcopy(net).forward_maxpool(x, start=start))
        assert names.count(FWD) == (1 if start else 3), names
        emu = _emulation(net, x, start)
    assert out16.dtype == BF and out32.dtype == torch.float32 and out16.shape == out32.shape == emu.shape
    d_own, d_emu = _rel_rms(out16.float(), out32), _rel_rms(emu, out32)
    tol = max(1.5 * d_emu, 1e-3)
    print("shared MLP %s: bf16 vs fp32 rel rms %.3e, emulation on the fp32 route %.3e" % (spec, d_own, d_emu))
    record_error("wide shared MLP %s bf16 vs fp32 (rel rms)" % (spec,), d_own, 1.0, tol)
    record_error("wide shared MLP %s emulation vs fp32 (rel rms)" % (spec,), d_emu, 1.0, tol)
    assert d_emu > 0
    assert d_own <= tol, (d_own, d_emu)


def _chain_bound(ref, x64, pool):
    """Per-element bound of the fused bf16 route against the float64 chain ``ref`` on the same bf16 input, built like
    test_mlp_eval_gpu._bf16_chain_bounds: 2^-8 (|value| + E) per rounding to bf16 -- here also the activated conv input and the
    weight, which the bf16-MFMA kernels round -- carried through the layers: a conv maps E to |W| E, an eval BatchNorm to
    |scale| E, ReLU and max are 1-Lipschitz; the fp32 arithmetic in between adds gamma(2 (Cin + 2)) |W| |a| per conv and
    8 u (|scale| (|v| + |mean|) + |beta|) per BatchNorm.  Every hidden conv output is stored once, the final tensor once."""
    v, e = x64, torch.zeros_like(x64)
    layers = list(ref)
    for k, layer in enumerate(layers):
        if isinstance(layer, nn.Conv2d):
            w = layer.weight.view(layer.out_channels, layer.in_channels).abs()
            if k > 0:
                e = e + BF16_EPS * (v.abs() + e)                                        # the activated input, rounded
            a = v.abs() + e
            g = 2 * (layer.in_channels + 2) * U
            z = layer(v)
            e = torch.einsum("oi,bims->boms", w, e + (BF16_EPS + g / (1 - g)) * a)      # + the weight's rounding + the accumulation
            if any(isinstance(t, nn.Conv2d) for t in layers[k + 1:]):
                e = e + BF16_EPS * (z.abs() + e)                                        # the conv output is stored in bf16
            v = z
        elif isinstance(layer, nn.BatchNorm2d):
            sc = (layer.weight / torch.sqrt(layer.running_var + layer.eps)).view(1, -1, 1, 1).abs()
            e = sc * e + 8 * U * (sc * (v.abs() + layer.running_mean.view(1, -1, 1, 1).abs()) + layer.bias.view(1, -1, 1, 1).abs())
            v = layer(v)
        else:
            v = torch.relu(v)
    if pool:
        v, e = v.max(dim=3).values, e.max(dim=3).values
    return v, e + BF16_EPS * (v.abs() + e)


@pytest.mark.parametrize("spec,start,cin,pool", [((99, 64, 64, 128), 1, 64, True), ((192, 128, 128), 1, 128, False),
                                                 ((128, 128, 256), 0, 128, True)], ids=["sa2_pooled", "fp_tail", "sa3_pooled"])
def test_eval_mode_drift_against_the_float64_chain(spec, start, cin, pool, monkeypatch):
    """Measured on an MI355X, max err at max |truth|, max err / bound: sa2_pooled 2.27e-2 at 4.25, 0.074; fp_tail 2.16e-2 at 6.42,
    0.366; sa3_pooled 3.11e-2 at 6.32, 0.056."""
    _on(monkeypatch)
    net = _mlp(spec, seed=9).eval()
    g = torch.Generator().manual_seed(12)
    x = torch.randn((2, cin, 1024, 32), generator=g).to(BF)
    ref = nn.Sequential(*list(copy.deepcopy(net).cpu().double())[start:])
    with torch.no_grad():
        truth, bound = _chain_bound(ref, x.double(), pool)
    log = _CallLog(monkeypatch)
    xd = x.cuda()
    with torch.no_grad():
        got, names = _run(log, (lambda: net.forward_maxpool(xd, start=start)) if pool else (lambda: net._run(xd, False, start=start)[0]))
    assert len(_wide(names)) >= 1 and not any(n.startswith("mgar_bn_act") for n in names), names
    assert names.count(POOL) == (1 if pool else 0)
    err = (got.double().cpu() - truth).abs()
    used = (err / bound).max().item()
    print("eval shared MLP %s: max err %.3e at max |truth| %.3e, max err / bound %.3f" % (spec, err.max().item(),
                                                                                          truth.abs().max().item(), used))
    record_error("wide eval shared MLP %s vs float64 chain (share of bound)" % (spec,), used, 1.0, 1.0)
    assert used <= 1.0, used
