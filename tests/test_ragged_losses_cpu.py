"""losses.mgar_losses_ragged -- the batched objective with validity masks -- against the looped mgar_losses(...,
person_num=counts) it restates: every supported Loss, both reference_semantics values, values and gradients with respect to
the 15 outputs that enter the objective, at 1e-6 relative (the terms are the same; only the summation shape differs)."""
import numpy as np
import pytest
import torch

MAX = 8
LOSSES = ("L_total", "L_act", "L_bce", "L_bce2")
TERMS = ("L_bce", "L_bce2", "L_pose", "L_interaction", "L_act", "SG_L_pose", "SG_L_interaction", "SG_L_act", "L_total")


def _fake_outputs(seed, batch, counts):
    """The model's 16-tuple: sigmoid-range heads, pose heads as the softmax the model emits, zero-padded beyond each count."""
    g = torch.Generator().manual_seed(seed)
    sig = lambda *s: torch.rand(*s, generator=g) * 0.98 + 0.01          # noqa: E731
    res = [sig(batch, MAX, MAX)] + [torch.softmax(torch.randn(batch, MAX, 4, generator=g), -1) for _ in range(3)] \
        + [sig(batch, MAX, k) for k in (2, 4, 7, 5)] + [sig(batch, MAX, 4) for _ in range(3)] + [sig(batch, MAX, k) for k in (2, 4, 7, 5)] \
        + [torch.rand(batch, 1, generator=g) * 4]
    for b, n in enumerate(counts):
        res[0][b, n:] = 0; res[0][b, :, n:] = 0
        for t in res[1:15]:
            t[b, n:] = 0
    return [t.requires_grad_(True) for t in res]


def _labels(counts, seed=4):
    rng = np.random.default_rng(seed)
    batch = len(counts)
    pid = -np.ones((batch, MAX), np.int64); gid = -np.ones((batch, MAX), np.int64)
    for b, n in enumerate(counts):
        pid[b, :n] = rng.permutation(40)[:n]
        gid[b, :n] = rng.integers(0, 3, n)
        gid[b, 0], gid[b, 1] = 0, 1
    action = torch.from_numpy((rng.random((batch, MAX, 27)) < 0.3).astype(np.float32))
    sga = torch.from_numpy((rng.random((batch, MAX, 27)) < 0.3).astype(np.float32))
    return torch.from_numpy(pid), torch.from_numpy(gid), action, sga


def _close(a, b, what):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-6 * scale + 1e-12, (what, err, scale)


@pytest.mark.parametrize("counts", [[2, 5, 3], [4, 4, 4]])
@pytest.mark.parametrize("ref_sem", [True, False])
@pytest.mark.parametrize("Loss", LOSSES)
def test_ragged_losses_equal_the_looped_losses(counts, ref_sem, Loss):
    from multimodal_gar_amd import losses
    pid, gid, action, sga = _labels(counts)
    res = _fake_outputs(21, len(counts), counts)
    looped = losses.mgar_losses(res, pid, gid, action, sga, Loss=Loss, person_num=counts, reference_semantics=ref_sem)
    ragged = losses.mgar_losses_ragged(res, gid, action, sga, counts, Loss=Loss, reference_semantics=ref_sem)
    assert set(ragged) == set(TERMS)
    for k in TERMS:
        _close(ragged[k], looped[k], k)
    ga = torch.autograd.grad(looped["L_total"], res[:15], allow_unused=True)
    gb = torch.autograd.grad(ragged["L_total"], res[:15], allow_unused=True)
    for i, (a, b) in enumerate(zip(gb, ga)):
        if b is None:                                   # an output outside this objective: no gradient, or an exact zero one
            assert a is None or not a.any(), i
            continue
        _close(a, b, "grad of output %d" % i)
        for s, n in enumerate(counts):                  # nothing flows into the padding
            assert not a[s, n:].any()
    if len(set(counts)) == 1:
        uniform = losses.mgar_losses_uniform(res, gid, action, sga, counts[0], Loss=Loss, reference_semantics=ref_sem)
        for k in TERMS:
            _close(ragged[k], uniform[k], "uniform " + k)
        gu = torch.autograd.grad(uniform["L_total"], res[:15], allow_unused=True)
        gr = torch.autograd.grad(losses.mgar_losses_ragged(res, gid, action, sga, counts, Loss=Loss,
                                                           reference_semantics=ref_sem)["L_total"], res[:15], allow_unused=True)
        for i, (a, b) in enumerate(zip(gr, gu)):
            if b is not None:
                _close(a, b, "uniform grad of output %d" % i)


def test_ragged_losses_mask_cache_and_no_loop_artefacts():
    """A second call with the same counts reuses the masks; garbage in the padded label slots changes nothing."""
    from multimodal_gar_amd import losses
    counts = [2, 5, 3]
    pid, gid, action, sga = _labels(counts)
    res = _fake_outputs(3, 3, counts)
    a = losses.mgar_losses_ragged(res, gid, action, sga, counts)
    key = (tuple(counts), "cpu")
    masks = losses._RAGGED_MASKS[key]
    gid2, action2 = gid.clone(), action.clone()
    for s, n in enumerate(counts):
        gid2[s, n:] = 7; action2[s, n:] = 1.0
    b = losses.mgar_losses_ragged(res, gid2, action2, sga, counts)
    assert losses._RAGGED_MASKS[key] is masks
    for k in TERMS:
        assert torch.equal(a[k], b[k]), k
