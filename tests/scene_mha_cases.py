"""Case table, seeded inputs and the float64 reference of the per-scene multi-head attention core
(mgar_scene_mha_fwd / _bwd of csrc/scene_mha.hip; scene_mha_ops.scene_mha):

    for every scene s and head h, with Q / K / V the head's 64 columns of the scene's rows:
    Att = softmax(Q K^T * scale, dim=1),  out = Att V.

Shapes: the smallest that reach every code path of the kernels -- one wave per (row, head), 4 rows per block; lanes along j
hold MGAR_DAFM_MAX_N / 64 = 2 columns each; q, k, v at a leading dimension of their own.  Also the names shared by the
generator and the tests of tests/golden/reference_fusion_table.npz."""
import os

import numpy as np
import torch

HEAD_DIM = 64
# ld: leading dimension of q, k, v in floats; fused: q, k, v are the three column slices of ONE (rows, ld) buffer
CASES = {
    "n1_n64_n65_H2": dict(counts=[1, 64, 65, 2], H=2, ld=128),                 # n = 1; the second column register starts
    "n128_n127_H8_fused": dict(counts=[128, 127, 3], H=8, ld=1536, fused=True),  # full capacity; 258 rows: partial last block
    "empty_scenes_H1": dict(counts=[5, 0, 7, 0], H=1, ld=64),                  # empty scenes mid-batch and at the end
    "large_logits_H8": dict(counts=[33], H=8, ld=512, qk_scale=4.0),           # large logits through the exponential
}
RTOL, ATOL = 1e-4, 1e-5     # the DAFM op tests' own values (tests/dafm_prior_cases.py)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fusion_table.npz")
# tests/golden/make_reference_fusion_table_golden.py
THRESHOLD_GAP = 1e-3        # THRESHOLD_GAP of tests/dafm_prior_cases.py
NET_COUNTS = ((5, 5, 5), (2, 7, 4))
# configuration name -> overrides of the shipped GAR_MODEL configuration (make_reference_golden.gar_cfg)
CONFIGS = {
    "crossAtt": dict(FUSION="crossAtt"),
    "catandAtt": dict(FUSION="catandAtt"),
    "RGB": dict(MODALITY="RGB", FEAT_NORM=False, FEATURE_DIM=512),
    "LiDAR": dict(MODALITY="LiDAR", FEAT_NORM=False, FEATURE_DIM=512),
}
LAYER_N, LAYER_SEED, LAYER_FILL_SEED = 9, 4321, 4


def inputs(counts, H, qk_scale=1.0, seed=11):
    """q, k, v (rows, 64 H) and the upstream gradient, fp32 on the CPU -- drawn like dafm_prior_cases.inputs."""
    g = torch.Generator().manual_seed(seed)
    rows, D = sum(counts), H * HEAD_DIM
    q = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    k = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    v = torch.randn(rows, D, generator=g)
    grad = torch.randn(rows, D, generator=g)
    return q, k, v, grad


def mha_reference(q, k, v, counts, H, scale, grad=None):
    """float64 over all scenes and heads: out (rows, 64 H), att (H, pairs) with each head's plane packed scene by scene,
    and, with an upstream gradient, dq, dk, dv."""
    qd, kd, vd = (t.detach().double().requires_grad_(grad is not None) for t in (q, k, v))
    rows = sum(counts)
    outs, atts, r0 = [], [[] for _ in range(H)], 0
    for n in counts:
        if n:
            heads = []
            for h in range(H):
                c = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
                a = torch.softmax(qd[r0:r0 + n, c] @ kd[r0:r0 + n, c].T * scale, dim=1)
                heads.append(a @ vd[r0:r0 + n, c])
                atts[h].append(a.detach().reshape(-1))
            outs.append(torch.cat(heads, dim=1))
        r0 += n
    out = torch.cat(outs) if outs else qd.new_zeros(rows, H * HEAD_DIM)
    att = torch.stack([torch.cat(a) if a else qd.new_zeros(0) for a in atts])
    if grad is None:
        return out.detach(), att
    out.backward(grad.double())
    return out.detach(), att, qd.grad, kd.grad, vd.grad


def threshold_gap(A, counts):
    """Smallest |A_theta - 0.5| over the valid off-diagonal entries of a padded (S, MNP, MNP) A_theta."""
    gap = np.inf
    for s, n in enumerate(counts):
        blk = np.asarray(A[s, :n, :n], np.float64)
        gap = min(gap, np.abs(blk[~np.eye(n, dtype=bool)] - 0.5).min())
    return float(gap)


def derived_counts(counts, mnp):
    """The counts get_num_person derives: a scene with no -1 slot counts one actor short (len(unique) - 1)."""
    return tuple(c - 1 if c == mnp else c for c in counts)


def net_tag(config, counts, mode):
    return "net_%s_%s_%s" % (config, "".join(str(c) for c in counts), mode)


def check_fixture(G):
    """The generator's assertions, on the arrays of the fixture: all 16 outputs of the 16 runs present and finite, no valid
    off-diagonal entry of A_theta within THRESHOLD_GAP of 0.5, running statistics of the FEAT_NORM train runs, the layer
    block.  Returns the smallest gap."""
    gaps = []
    for config, over in CONFIGS.items():
        for counts in NET_COUNTS:
            for mode in ("eval", "train"):
                tag = net_tag(config, counts, mode)
                for i in range(16):
                    assert np.isfinite(G["%s_%02d" % (tag, i)]).all(), (tag, i)
                A = G[tag + "_00"]
                gap = threshold_gap(A, derived_counts(counts, A.shape[1]))
                assert gap > THRESHOLD_GAP, (tag, gap)
                gaps.append(gap)
                has_stats = mode == "train" and over.get("FEAT_NORM", True)
                for bn in ("bn_rgb", "bn_lidar"):
                    for stat in ("mean", "var"):
                        key = "%s_%s_%s" % (tag, bn, stat)
                        assert (key in G) == has_stats, key
                        if has_stats:
                            assert G[key].shape == (512,) and np.isfinite(G[key]).all(), key
    for key in ("layer_R", "layer_L", "layer_out"):
        assert G[key].shape == (LAYER_N, 512) and np.isfinite(G[key]).all(), key
    return min(gaps)
