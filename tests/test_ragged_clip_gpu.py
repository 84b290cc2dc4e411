"""ClipModel on a batch whose clips hold different numbers of actors (make_batch(..., actor_counts=...)): RoI lift of the
valid boxes only, packed tokens, the fusion net's ragged batched route and the masked objective, against the same model
with GAR_MODEL.DISABLE_BATCHED (the per-scene loop and, for the objective, the looped mgar_losses), within the caps of the
route tests (2e-4 of each tensor's largest entry)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu

A, POINTS, COUNTS = 5, 1024, [3, 5]


def _model(train):
    from multimodal_gar_amd import workload as W
    torch.manual_seed(0)
    model = fill_deterministic(W.ClipModel(A, POINTS), seed=11).train(train)
    model.batch_i3d = train          # several clips in one I3D pass need batch statistics: eval goes clip by clip
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    return model.cuda()


def _batch(actor_counts=None):
    from multimodal_gar_amd import workload as W
    return W.make_batch(5, 2, 2, A, POINTS, 64, 96, torch.device("cuda"), actor_counts=actor_counts)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_ragged_clip_serial_schedule_equals_per_scene_route(mode):
    from multimodal_gar_amd import losses, workload as W
    from multimodal_gar_amd.model.gat_model import GAR_Fusion_Net3
    batch = _batch(COUNTS)
    ragged = _model(mode == "train")
    ragged.overlap_branches = False                      # the serial schedule
    per = copy.deepcopy(ragged)
    per.net.GAR_model.cfg.DISABLE_BATCHED = True
    taken = []
    real = GAR_Fusion_Net3.forward_packed
    try:
        GAR_Fusion_Net3.forward_packed = lambda self, *a, **k: (taken.append(1), real(self, *a, **k))[1]
        with torch.no_grad():
            got, want = ragged(batch), per(batch)
    finally:
        GAR_Fusion_Net3.forward_packed = real
    assert taken == [1] and len(got) == len(want) == 16
    frames = [c for c in COUNTS for _ in range(2)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape
        print("%s output %d: %.3e" % (mode, i, _rel(g, w)))
        assert _rel(g, w) <= 2e-4, i
        if i < 15:
            for s, n in enumerate(frames):
                assert not g[s, n:].any()
    loss = W.reference_loss(got, batch)
    looped = losses.mgar_losses(want, batch["person_id"], batch["social_group_id"], batch["action"], batch["social_group_activity"],
                                Loss="L_total", person_num=frames, reference_semantics=False)["L_total"]
    print("%s loss %.6f vs %.6f" % (mode, float(loss), float(looped)))
    assert abs(float(loss) - float(looped)) <= 2e-4 * abs(float(looped))


def test_full_counts_equal_the_batch_without_the_key():
    model = _model(True)             # batch statistics and no dropout: a second pass gives the first one's bits
    model.overlap_branches = False
    plain, full = _batch(), _batch([A, A])
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(v, full[k]), k
    with torch.no_grad():
        want, got = model(plain), model(full)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), i


def test_ragged_clip_training_step_under_the_forked_schedule():
    from multimodal_gar_amd import workload as W
    model = _model(True)
    assert model.overlap_branches
    batch = _batch(COUNTS)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    before = model.net.GAR_model.D_embed[0].weight.detach().clone()
    loss = W.reference_loss(model(batch), batch)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert not torch.equal(before, model.net.GAR_model.D_embed[0].weight)


def test_ragged_objective_does_not_synchronise():
    """reference_loss on a ragged batch, forward and backward: after one warm-up call (which builds the masks of the count
    list) a second call reads nothing from and copies nothing to the host."""
    from multimodal_gar_amd import workload as W
    batch = _batch(COUNTS)
    g = torch.Generator(device="cuda").manual_seed(3)
    S, M = 4, A + 1
    sig = lambda *s: (torch.rand(*s, device="cuda", generator=g) * 0.98 + 0.01).requires_grad_(True)      # noqa: E731
    outs = [sig(S, M, M)] + [sig(S, M, 4) for _ in range(3)] + [sig(S, M, k) for k in (2, 4, 7, 5)] \
        + [sig(S, M, 4) for _ in range(3)] + [sig(S, M, k) for k in (2, 4, 7, 5)] + [sig(S, 1)]
    W.reference_loss(outs, batch).backward()             # warm-up
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        loss = W.reference_loss(outs, batch)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.isfinite(loss).all() and all(torch.isfinite(o.grad).all() for o in outs[:15])
