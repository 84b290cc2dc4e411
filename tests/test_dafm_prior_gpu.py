"""dafm_ops.dafm_attention_add (csrc/dafm.hip, the additive-prior instantiation of the DAFM kernels) against the float64
reference of dafm_prior_cases.py (tests/test_dafm_prior_cpu.py shows that reference right): out, att, dq, dk, dv at
1e-4 relative to the largest reference value + 1e-5 (tests/test_fusion_edges_gpu.py; BASELINE.json north_star), every att
row summing to 1 within 1e-5, masked entries exactly 0; and the layers built on it against the reference's own outputs
(tests/golden/reference_fusion_variants.npz) at the tolerance of test_reference_blocks.test_dafm_layer_matches_reference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import dafm_prior_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(PC.GOLDEN)


def close(a, b, what, rtol=PC.RTOL, atol=PC.ATOL):
    a = a.detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    print("%s: err %.3e scale %.3e" % (what, err, scale))
    assert err <= atol + rtol * scale, "%s: max err %g vs scale %g" % (what, err, scale)


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(inputs, prior blocks, float64 reference) -- computed once per case, never modified."""
    case = PC.CASES[name]
    q, k, v, g = PC.inputs(case["counts"], case["D"], case.get("qk_scale", 1.0))
    blocks = PC.prior(kind, case["counts"])
    return (q, k, v, g), blocks, PC.reference(q, k, v, blocks, case["counts"], 1.0 / case["D"] ** 0.5, g)


def _device_run(q0, k0, v0, g, prior_flat, counts, scale, touch_att=False):
    from multimodal_gar_amd.dafm_ops import dafm_attention_add, scene_offsets
    q, k, v = (t.cuda().requires_grad_(True) for t in (q0, k0, v0))
    so, do = scene_offsets(counts, "cuda")
    out, att = dafm_attention_add(q, k, v, prior_flat, so, do, scale)
    assert out.requires_grad and not att.requires_grad
    loss = (out * g.cuda()).sum() + (att.sum() * 3.0 if touch_att else 0.0)
    loss.backward()
    return out.detach(), att, q.grad, k.grad, v.grad


@pytest.mark.parametrize("kind", PC.PRIORS)
@pytest.mark.parametrize("name", list(PC.CASES))
def test_attention_add_case(name, kind):
    counts, D = PC.CASES[name]["counts"], PC.CASES[name]["D"]
    (q0, k0, v0, g), blocks, (r_out, r_att, r_dq, r_dk, r_dv) = _case(name, kind)
    prior_flat = None if blocks is None else PC.flat(blocks).cuda()
    out, att, dq, dk, dv = _device_run(q0, k0, v0, g, prior_flat, counts, 1.0 / D ** 0.5)
    assert att.shape == (sum(n * n for n in counts),)
    close(out, r_out, "out"); close(att, r_att, "att")
    m0 = 0
    for n in counts:                                    # every row of every scene's att sums to 1
        if n:
            rows = att[m0:m0 + n * n].view(n, n).sum(1)
            assert (rows - 1).abs().max().item() <= 1e-5, (n, (rows - 1).abs().max().item())
        m0 += n * n
    if kind == "masked":
        hidden = PC.flat(blocks) == PC.MASK_VALUE
        assert hidden.any() and not att.cpu()[hidden].any()
        assert not r_att[hidden].any()
    close(dq, r_dq, "dq"); close(dk, r_dk, "dk"); close(dv, r_dv, "dv")


def test_no_prior_and_a_prior_of_zeros_give_the_same_bits():
    counts, D = [6, 65, 3], 128
    q0, k0, v0, g = PC.inputs(counts, D, seed=13)
    zeros = torch.zeros(sum(n * n for n in counts), device="cuda")
    a = _device_run(q0, k0, v0, g, None, counts, 0.125)
    b = _device_run(q0, k0, v0, g, zeros, counts, 0.125)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_with_the_pair_count_passed_nothing_is_read_from_the_device():
    """pairs = sum n_s^2 from the caller (scene_layout().pairs on the batched route): the same bits as with the count read
    back from the offsets, and no synchronisation -- also with offsets that are copies of the cached ones."""
    from multimodal_gar_amd.dafm_ops import dafm_attention_add, scene_offsets
    counts, D = [6, 0, 3], 64
    q, k, v, _ = (t.cuda() for t in PC.inputs(counts, D, seed=16))
    prior_flat = PC.flat(PC.prior("seeded", counts)).cuda()
    so, do = (t.clone() for t in scene_offsets(counts, "cuda"))
    want = dafm_attention_add(q, k, v, prior_flat, so, do, 0.125)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        got = dafm_attention_add(q, k, v, prior_flat, so, do, 0.125, pairs=45)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="prior"):
        dafm_attention_add(q, k, v, prior_flat, so, do, 0.125, pairs=44)


def test_att_is_not_differentiable_and_out_gradients_are_unchanged():
    counts, D = [6, 3], 64
    q0, k0, v0, g = PC.inputs(counts, D, seed=14)
    prior_flat = PC.flat(PC.prior("seeded", counts)).cuda()
    a = _device_run(q0, k0, v0, g, prior_flat, counts, 0.125, touch_att=False)
    b = _device_run(q0, k0, v0, g, prior_flat, counts, 0.125, touch_att=True)
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


def test_wrong_sized_prior_raises_before_any_launch():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import dafm_attention_add, scene_offsets
    counts, D = [6, 3], 64
    q, k, v, _ = (t.cuda() for t in PC.inputs(counts, D, seed=15))
    so, do = scene_offsets(counts, "cuda")
    launched = []
    real = L.call
    try:
        L.call = lambda name, *a: (launched.append(name), real(name, *a))[1]
        for numel in (6 * 6 + 3 * 3 - 1, 6 * 6 + 3 * 3 + 1, 9 * 9):
            with pytest.raises(ValueError, match="prior"):
                dafm_attention_add(q, k, v, torch.zeros(numel, device="cuda"), so, do, 0.125)
    finally:
        L.call = real
    assert launched == []


@pytest.mark.parametrize("name", list(PC.LAYERS))
def test_layer_on_the_device_matches_reference(name):
    """forward_stacked of each layer (one scene of 9 actors) against the outputs of the reference's own class."""
    from multimodal_gar_amd.dafm_ops import scene_offsets
    from multimodal_gar_amd.model import gat_model
    cls, sigma, outs = PC.LAYERS[name]
    layer = fill_deterministic(getattr(gat_model, cls)(input_dim=64, out_dim=64, sigma=sigma), seed=4).cuda().eval()
    R, L, De, Dg = (torch.from_numpy(G["layer_" + k]).cuda() for k in ("R", "L", "De", "Dg"))
    so, do = scene_offsets([R.shape[0]], "cuda")
    with torch.no_grad():
        res = layer.forward_stacked(R, L, De.reshape(-1), Dg.reshape(-1), so, do)
    res = (res,) if len(outs) == 1 else res
    assert len(res) == len(outs)
    for o, r in zip(outs, res):
        close(r, G["layer_%s_%s" % (name, o)], "%s %s" % (name, o), rtol=PC.LAYER_RTOL, atol=PC.LAYER_ATOL)
