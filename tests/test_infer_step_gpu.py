"""Device tests of workload.InferStep, the eval-mode whole-model step: eager against captured replay, the fused tail against the
same model with the switch off, the group ids it hands out, untouched BatchNorm buffers, which entry points an eval forward
reaches, the single-modality models, the voxel route and bf16."""
import numpy as np
import pytest
import torch

import scene_tail_cases as T
import test_bf16_gpu as B
from test_scene_tail_gpu import _Calls

pytestmark = pytest.mark.gpu

SHAPE = (2, 2, 5, 1024, 64, 96)          # clips, frames, actors, points, height, width
EVAL_ENTRIES = ("mgar_stem_conv3d_fwd_affine", "mgar_conv3d_k3_fwd_affine", "mgar_pointwise_conv_maxpool_eval_fwd",
                "mgar_nonlocal_dot_eval_fwd", "mgar_scene_tail_eval_fwd")


def _W():
    from multimodal_gar_amd import scene_tail_ops, workload
    return workload, scene_tail_ops


def _batch(actor_counts=None, seed=5):
    W, _ = _W()
    return W.make_batch(seed, *SHAPE, torch.device("cuda"), actor_counts=actor_counts)


def _bn_buffers(module):
    return {n: b.detach().clone() for n, b in module.named_buffers()
            if n.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}


def _frame_counts(batch):
    per_clip = batch.get("actor_counts") or [batch["n_actors"]] * batch["n_clips"]
    return [c for c in per_clip for _ in range(batch["n_frames"])]


def _check_group_ids(step, res, batch):
    counts = _frame_counts(batch)
    gar = step.module.net.GAR_model
    A, gid = res.outputs[0], res.group_id
    assert gid.shape == (len(counts), batch["n_actors"] + 1) and gid.dtype == torch.int32
    for s, n in enumerate(counts):
        assert torch.equal(gid[s, :n].long(), gar._predicted_groups(A[s, :n, :n])) and (gid[s, n:] == -1).all()


@pytest.mark.parametrize("actor_counts", [None, [5, 3]], ids=["uniform", "ragged"])
def test_eager_replay_switch_and_buffers(actor_counts, monkeypatch):
    W, O = _W()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    dev = torch.device("cuda", 0)
    step = W.InferStep(5, 1024, dev)
    assert not any(m.training for m in step.module.modules())
    batch = _batch(actor_counts)
    before = _bn_buffers(step.module)
    assert len(before) > 100
    with _Calls() as n:
        eager = step.run_eager(batch)
    torch.cuda.synchronize()
    assert isinstance(eager, W.Inference) and len(eager.outputs) == 16
    from multimodal_gar_amd import bn_ops
    # the shared-MLP kernel has a column threshold (bn_ops.EVAL_MIN_COLUMNS): at this shape only the RoI-grid lift of the full
    # batch reaches it -- 20 boxes x 216 grid points x 16 samples = 69 120 columns, 16 boxes give 55 296
    lift_columns = sum(_frame_counts(batch)) * 216 * 16
    for name in EVAL_ENTRIES:
        if name == "mgar_pointwise_conv_maxpool_eval_fwd" and lift_columns < bn_ops.EVAL_MIN_COLUMNS:
            assert actor_counts is not None and n.get(name, 0) == 0
            continue
        assert n.get(name, 0) >= 1, name
    assert n["mgar_scene_tail_eval_fwd"] == 1
    assert not [k for k in n if k.startswith("mgar_bn_train_stats")] and "mgar_scene_bn_fwd" not in n
    _check_group_ids(step, eager, batch)
    # the same model with the switch off: the previous route, ids from _predicted_groups
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", False)
    with _Calls() as n_off:
        off = step.run_eager(batch)
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    assert "mgar_scene_tail_eval_fwd" not in n_off
    _check_group_ids(step, off, batch)
    counts = _frame_counts(batch)
    bound = T.worst_case_value_bound(step.module.net.GAR_model.D_embed, 512)
    rows_ok = T.margin_rows(off.outputs[0].cpu().numpy(), counts, bound)
    err = float((eager.outputs[0].double() - off.outputs[0].double()).abs().max())
    print("InferStep %s: fused vs switch off max |dA| %.3g (bound %.3g), rows keeping the margin %.3f"
          % (actor_counts, err, bound, float(np.concatenate(rows_ok).mean())))
    assert err <= bound
    for i in range(1, 8):
        assert torch.equal(eager.outputs[i], off.outputs[i])
    for s, n_s in enumerate(counts):
        if torch.equal(eager.group_id[s], off.group_id[s]):
            for i in range(8, 15):
                assert torch.equal(eager.outputs[i][s], off.outputs[i][s])
        else:
            assert not rows_ok[s].all()
    # captured replay == eager, bit for bit
    kept = [o.clone() for o in eager.outputs] + [eager.group_id.clone()]
    step.capture(batch)
    assert step.graph is not None
    for _ in range(2):
        rep = step.run(batch)
        torch.cuda.synchronize()
        for a, b in zip(list(rep.outputs) + [rep.group_id], kept):
            assert torch.equal(a, b)
    after = _bn_buffers(step.module)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("modality", ["RGB", "LiDAR"])
def test_single_modality(modality, monkeypatch):
    W, O = _W()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    step = W.InferStep(5, 1024, torch.device("cuda", 0), modality=modality)
    batch = _batch([5, 3])
    before = _bn_buffers(step.module)
    with _Calls() as n:
        res = step.run_eager(batch)
    assert n.get("mgar_scene_tail_eval_fwd", 0) == 1 and len(res.outputs) == 16
    assert all(torch.isfinite(o).all() for o in res.outputs)
    _check_group_ids(step, res, batch)
    kept = [o.clone() for o in res.outputs] + [res.group_id.clone()]
    step.capture(batch)
    rep = step.run(batch)
    torch.cuda.synchronize()
    for a, b in zip(list(rep.outputs) + [rep.group_id], kept):
        assert torch.equal(a, b)
    after = _bn_buffers(step.module)
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_bf16_runs_and_keeps_the_indices():
    """The bf16 configuration of the eval step with the fp32 step's weights: every integer output of the query ops is identical
    (coordinates and distances stay fp32, as test_bf16_gpu.py establishes for the train-mode forward), the outputs are finite
    and the fusion net's entry points are the fp32 ones."""
    W, _ = _W()
    dev = torch.device("cuda", 0)
    steps = {p: W.InferStep(5, 1024, dev, precision=p, seed=9) for p in ("fp32", "bf16")}
    steps["bf16"].module.load_state_dict(steps["fp32"].module.state_dict())
    batch = _batch()
    logs, outs = {}, {}
    for p, st in steps.items():
        with B._IndexRecorder() as rec, _Calls() as n:
            outs[p] = st.run_eager(batch)
        torch.cuda.synchronize()
        logs[p] = rec.log
        assert n.get("mgar_scene_tail_eval_fwd", 0) == 1
        if p == "bf16":
            assert n.get("mgar_conv3d_k3_bf16_fwd_affine", 0) >= 1 and n.get("mgar_pointwise_conv_maxpool_eval_bf16_fwd", 0) >= 1
    assert len(logs["fp32"]) == len(logs["bf16"]) >= 10
    for (n1, t1), (n2, t2) in zip(logs["fp32"], logs["bf16"]):
        assert n1 == n2 and torch.equal(t1, t2), n1
    assert all(torch.isfinite(o).all() and o.dtype == torch.float32 for o in outs["bf16"].outputs)
    _check_group_ids(steps["bf16"], outs["bf16"], batch)


def test_voxel_route_is_eager_only():
    W, _ = _W()
    dev = torch.device("cuda", 0)
    step = W.InferStep(4, 4096, dev, route="voxel", seed=9)
    batch = W.make_batch(35, 1, 2, 4, 4096, 96, 160, dev)
    before = _bn_buffers(step.module)
    with _Calls() as n:
        res = step.run(batch)
    torch.cuda.synchronize()
    assert n.get("mgar_scene_tail_eval_fwd", 0) == 1 and n.get("mgar_voxel_roi_pool_eval_fwd", 0) >= 1
    assert n.get("mgar_spconv_gather_gemm_affine", 0) >= 1
    assert not [k for k in n if k.startswith("mgar_bn_train_stats")]
    assert all(torch.isfinite(o).all() for o in res.outputs)
    _check_group_ids(step, res, batch)
    if not W.voxel_route_capturable():
        with pytest.raises(RuntimeError):
            step.capture(batch)
        assert step.graph is None
    after = _bn_buffers(step.module)
    assert all(torch.equal(before[k], after[k]) for k in before)
