"""GAR_Fusion_Net3 on a batch whose scenes hold different numbers of actors: the ragged batched route (_forward_ragged, on
csrc/scene_ops.hip and the stacked DAFM layers) against the per-scene loop that the reference fixtures pin, on the network
of test_reference_blocks.test_gar_fusion_net3_routes_agree_in_gradients.

Tolerance: measured, not chosen.  The existing uniform batched route differs from the per-scene route on a uniform batch of
comparable size (S = 5, n = 12) by some max-norm figure (relative to each tensor's largest entry); the ragged route, which
sums in yet another order, may differ from the per-scene route by at most twice that, and never by more than the caps of
the existing route tests (2e-4 on outputs, 5e-4 on gradients).  Both figures are printed.  Measured on an MI355X
(uniform batched vs per-scene; ragged vs per-scene): eval outputs 6.2e-7; 5.7e-7 -- train outputs 6.8e-7; 6.3e-7 -- train
gradients 1.16e-6; 2.00e-6 (d rgb).  DESIGN.md section 5e."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = [2, 7, 33, 5, 12]
MNP = 35
SEED = 0
CAP_OUT, CAP_GRAD = 2e-4, 5e-4
GRAD_NAMES = ("rgb", "lidar", "AttFusModule1.WQ_r", "D_embed.0.weight", "card_net.0.weight")


def _gar_cfg(**extra):
    from multimodal_gar_amd.pcdet.config import EasyDict
    cfg = dict(MODALITY="Multi", FUSION="Attention_mat", SIGMA=10, FEAT_NORM=True, EUCLIDEAN=True,
               ind_action_concat=True, sg_feat_org=False, FEATURE_DIM=1024, HIDDEN_DIM=512, sim="cosine")
    cfg.update(extra)
    return EasyDict(**cfg)


def _net(train, **extra):
    from multimodal_gar_amd.model.gat_model import GAR_Fusion_Net3
    net = fill_deterministic(GAR_Fusion_Net3(_gar_cfg(**extra)), seed=5).cuda()
    net.train(train)
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return net


@functools.lru_cache(maxsize=None)
def _batch(counts, seed=SEED):
    """Seeded features and boxes (2-D boxes of positive area) with person_id = 0..n-1 in the leading slots and -1 behind."""
    g = torch.Generator().manual_seed(seed)
    S = len(counts)
    rgb, lid = torch.randn(S, MNP, 512, generator=g), torch.randn(S, MNP, 512, generator=g)
    xy = torch.rand(S, MNP, 2, generator=g) * 300
    bb = torch.cat((xy, xy + 5 + torch.rand(S, MNP, 2, generator=g) * 120), dim=2)
    b3 = torch.cat((torch.randn(S, MNP, 3, generator=g) * 4, torch.rand(S, MNP, 4, generator=g)), dim=2)
    pid = torch.full((S, MNP), -1, dtype=torch.int64)
    for s, n in enumerate(counts):
        pid[s, :n] = torch.arange(n)
    return tuple(t.cuda() for t in (rgb, lid, bb, b3, pid))


def _run(net, batch, grads=True):
    rgb, lid, bb, b3, pid = batch
    r, l = rgb.clone().requires_grad_(grads), lid.clone().requires_grad_(grads)
    with torch.set_grad_enabled(grads):
        res = net(r, l, bb, b3, None, pid)
    out = {"out%02d" % i: o.detach() for i, o in enumerate(res)}
    for bn in ("bn_rgb", "bn_lidar"):
        out[bn + ".running_mean"] = getattr(net, bn).running_mean.clone()
        out[bn + ".running_var"] = getattr(net, bn).running_var.clone()
    out["nbt"] = (int(net.bn_rgb.num_batches_tracked), int(net.bn_lidar.num_batches_tracked))
    g = {}
    if grads:
        sum((o * o).sum() for o in res).backward()
        g = dict(zip(GRAD_NAMES, (r.grad, l.grad, net.AttFusModule1.WQ_r.grad, net.D_embed[0].weight.grad,
                                  net.card_net[0].weight.grad)))
    return out, g


def _rel(a, b):
    """max-norm difference relative to the comparator's largest entry."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _worst(got, want):
    return max((_rel(got[k], want[k]), k) for k in want if k != "nbt")


@functools.lru_cache(maxsize=None)
def _routes(counts, train):
    """(per-scene, batched) results on the same inputs; which batched route runs follows from the counts."""
    batch = _batch(counts)
    per = _run(_net(train, DISABLE_BATCHED=True), batch, grads=train)
    bat = _run(_net(train), batch, grads=train)
    return per, bat


@functools.lru_cache(maxsize=None)
def _measured(train):
    """What the existing uniform batched route differs from the per-scene route by on S = 5, n = 12."""
    (po, pg), (bo, bg) = _routes((12,) * 5, train)
    return _worst(bo, po)[0], (_worst(bg, pg)[0] if train else 0.0)


def test_precondition_no_adjacency_entry_near_the_threshold():
    """On the per-scene route's A_theta no valid off-diagonal entry lies within 1e-3 of 0.5: the predicted groups cannot
    flip between two routes that differ by rounding, so a failure below is a failure of the arithmetic."""
    for train in (False, True):
        for counts in (tuple(COUNTS), (12,) * 5):
            A = _routes(counts, train)[0][0]["out00"]
            for s, n in enumerate(counts):
                blk = A[s, :n, :n]
                off = ~torch.eye(n, dtype=torch.bool, device=blk.device)
                gap = float((blk[off] - 0.5).abs().min())
                assert gap > 1e-3, (train, counts, s, gap)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_ragged_route_equals_per_scene_route(mode):
    train = mode == "train"
    d_out, d_grad = _measured(train)
    (po, pg), (ro, rg) = _routes(tuple(COUNTS), train)
    w_out = _worst(ro, po)
    print("%s outputs: uniform batched vs per-scene %.3e; ragged vs per-scene %.3e (%s)" % (mode, d_out, w_out[0], w_out[1]))
    assert len([k for k in ro if k.startswith("out")]) == 16
    assert ro["nbt"] == po["nbt"] and (not train or po["nbt"] == (len(COUNTS),) * 2)
    for s, n in enumerate(COUNTS):                       # padded slots are exactly zero
        assert not ro["out00"][s, n:].any() and not ro["out00"][s, :, n:].any()
        for i in range(1, 15):
            assert not ro["out%02d" % i][s, n:].any(), i
    assert w_out[0] <= min(2 * d_out, CAP_OUT), w_out
    if train:
        w_grad = _worst(rg, pg)
        print("train gradients: uniform batched vs per-scene %.3e; ragged vs per-scene %.3e (%s)" % (d_grad, w_grad[0], w_grad[1]))
        for s, n in enumerate(COUNTS):
            assert not rg["rgb"][s, n:].any() and not rg["lidar"][s, n:].any()
        assert w_grad[0] <= min(2 * d_grad, CAP_GRAD), w_grad


def test_ragged_batch_takes_the_ragged_route_and_promise_changes_no_bit():
    from multimodal_gar_amd.model.gat_model import GAR_Fusion_Net3
    batch = _batch(tuple(COUNTS))
    calls = []
    real = {name: getattr(GAR_Fusion_Net3, name) for name in ("_forward_ragged", "forward_per_scene", "_forward_batched")}
    try:
        for name, fn in real.items():
            setattr(GAR_Fusion_Net3, name, (lambda name, fn: lambda self, *a, **k: (calls.append(name), fn(self, *a, **k))[1])(name, fn))
        derived = _run(_net(True), batch)
        net = _net(True)
        net.actor_counts = list(COUNTS)
        promised = _run(net, batch)
    finally:
        for name, fn in real.items():
            setattr(GAR_Fusion_Net3, name, fn)
    assert calls == ["_forward_ragged", "_forward_ragged"]
    for a, b in zip(derived, promised):
        for k in a:
            assert a[k] == b[k] if k == "nbt" else torch.equal(a[k], b[k]), k


def test_ragged_route_does_not_synchronise_with_the_promise():
    batch = _batch(tuple(COUNTS))
    net = _net(True)
    net.actor_counts = list(COUNTS)
    rgb, lid, bb, b3, pid = batch
    r, l = rgb.clone().requires_grad_(True), lid.clone().requires_grad_(True)

    def step():
        res = net(r, l, bb, b3, None, pid)
        sum((o * o).sum() for o in res).backward()
    step()                                               # warm-up: builds and caches the layout
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.isfinite(r.grad).all()


def _route_taken(net, batch):
    """Name of the route forward() takes, without running it."""
    class Taken(Exception):
        pass
    cls = type(net)
    real = {name: getattr(cls, name) for name in ("_forward_ragged", "forward_per_scene", "_forward_batched")}

    def stop(name):
        def f(self, *a, **k):
            raise Taken(name)
        return f
    try:
        for name in real:
            setattr(cls, name, stop(name))
        with pytest.raises(Taken) as e:
            net(*batch[:4], None, batch[4])
    finally:
        for name, fn in real.items():
            setattr(cls, name, fn)
    return str(e.value)


def test_fallbacks_still_go_per_scene():
    rgb, lid, bb, b3, pid = _batch(tuple(COUNTS))
    one = pid.clone(); one[3, 1:] = -1                                       # a scene of one actor
    assert _route_taken(_net(False), (rgb, lid, bb, b3, one)) == "forward_per_scene"
    net = _net(False); net.actor_counts = [2, 7, 33, 1, 12]
    assert _route_taken(net, (rgb, lid, bb, b3, one)) == "forward_per_scene"
    hole = pid.clone(); hole[1, 2] = -1                                      # a hole in the valid slots
    assert _route_taken(_net(False), (rgb, lid, bb, b3, hole)) == "forward_per_scene"
    assert _route_taken(_net(False, sg_feat_org=True), (rgb, lid, bb, b3, pid)) == "forward_per_scene"   # not the shipped configuration
    assert _route_taken(_net(False, DISABLE_BATCHED=True), (rgb, lid, bb, b3, pid)) == "forward_per_scene"
    assert _route_taken(_net(False), (rgb, lid, bb, b3, pid)) == "_forward_ragged"


@pytest.mark.parametrize("promise", [None, "actor_counts", "uniform_actor_count"])
def test_uniform_batch_still_takes_the_uniform_route_bit_for_bit(promise):
    batch = _batch((12,) * 5)
    rgb, lid, bb, b3, pid = batch
    net = _net(True)
    if promise == "actor_counts":
        net.actor_counts = [12] * 5
    elif promise:
        net.uniform_actor_count = 12
    assert _route_taken(net, batch) == "_forward_batched"
    got, _ = _run(net, batch, grads=False)
    ref = _net(True)
    with torch.no_grad():
        want = ref._forward_batched(rgb, lid, bb, b3, pid)
    for i, w in enumerate(want):
        assert torch.equal(got["out%02d" % i], w), i
    assert torch.equal(net.bn_rgb.running_var, ref.bn_rgb.running_var)
