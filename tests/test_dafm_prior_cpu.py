"""The attention core with an additive prior (csrc/dafm.hip, mgar_dafm_attn_add_*) -- what can be pinned without a GPU.

The device tests (tests/test_dafm_prior_gpu.py, tests/test_fusion_variants_gpu.py) judge the kernels by the float64
reference of dafm_prior_cases.py and by tests/golden/reference_fusion_variants.npz.  Here, with no kernel involved:

* that float64 reference is the arithmetic of `_TwoBranchFusion._attend` (the per-scene mirror of the reference's layers) for
  a layer without a prior and for one with an additive prior;
* the layer-level fixtures, which the reference's own classes wrote, are reproduced by this package's modules on the CPU;
* what the fixture generator asserted holds for the committed file: finite outputs, no valid off-diagonal A_theta entry
  within 1e-3 of the grouping threshold, and every prior moving its layer's output by more than 100 x the layer tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

import dafm_prior_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

G = np.load(PC.GOLDEN)


@pytest.mark.parametrize("kind", [None, "add"])
def test_float64_reference_is_the_arithmetic_of_the_per_scene_layer(kind):
    from multimodal_gar_amd.model.gat_model import _TwoBranchFusion
    layer = _TwoBranchFusion(64, 64)
    n = 9
    q, k, v, _ = (t.double() for t in PC.inputs([n], 64))
    p = PC.prior("seeded", [n])[0].double() if kind else None
    want = layer._attend(q, k, v, kind, p)
    got, att = PC.attention_add_ref(q, k, v, p, 1.0 / 64 ** 0.5)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(att.sum(1), torch.ones(n, dtype=torch.float64), rtol=0, atol=1e-12)
    if kind:                                             # and the prior is not a no-op in the reference
        assert (got - PC.attention_add_ref(q, k, v, None, 1.0 / 64 ** 0.5)[0]).abs().max() > 1e-2


def _close(a, b, rtol=PC.LAYER_RTOL, atol=PC.LAYER_ATOL):
    a, b = a.detach().double().cpu().numpy(), np.asarray(b, np.float64)
    assert a.shape == b.shape
    err, scale = np.abs(a - b).max(), np.abs(b).max() + 1e-12
    assert err <= atol + rtol * scale, "max err %g vs scale %g" % (err, scale)


@pytest.mark.parametrize("name", list(PC.LAYERS))
def test_layer_fixture_is_reproduced_by_the_per_scene_module(name):
    from multimodal_gar_amd.model import gat_model
    cls, sigma, outs = PC.LAYERS[name]
    layer = fill_deterministic(getattr(gat_model, cls)(input_dim=64, out_dim=64, sigma=sigma), seed=4).eval()
    R, L, De, Dg = (torch.from_numpy(G["layer_" + k]) for k in ("R", "L", "De", "Dg"))
    with torch.no_grad():
        res = layer(R, L, Dg, De)
    res = (res,) if len(outs) == 1 else res
    assert len(res) == len(outs)
    for o, r in zip(outs, res):
        _close(r, G["layer_%s_%s" % (name, o)])


def test_committed_fixture_keeps_what_its_generator_asserted():
    assert all(np.isfinite(G[k]).all() for k in G.files)
    gaps = []
    for fusion in PC.FUSIONS:
        for counts in PC.NET_COUNTS:
            for mode in ("eval", "train"):
                tag = PC.net_tag(fusion, counts, mode)
                assert all("%s_%02d" % (tag, i) in G.files for i in range(16)), tag
                gaps.append(PC.threshold_gap(G[tag + "_00"], counts))
                if mode == "train":
                    assert all("%s_%s_%s" % (tag, bn, st) in G.files for bn in ("bn_rgb", "bn_lidar") for st in ("mean", "var"))
    assert min(gaps) > PC.THRESHOLD_GAP, min(gaps)
    for name, (_, _, outs) in PC.LAYERS.items():
        if name == "plain":
            continue
        for o in outs:
            out, bare = (np.asarray(G["layer_%s_%s%s" % (name, mid, o)], np.float64) for mid in ("", "noprior_"))
            assert np.abs(out - bare).max() > 100 * (PC.LAYER_RTOL * np.abs(out).max() + PC.LAYER_ATOL), (name, o)
