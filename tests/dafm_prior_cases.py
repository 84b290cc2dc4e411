"""Case table, seeded inputs and the float64 reference of the attention core with an ADDITIVE prior on the logits
(mgar_dafm_attn_add_fwd / _bwd of csrc/dafm.hip; dafm_ops.dafm_attention_add):

    Att = softmax(q k^T * scale + P, dim=1),  out = Att v,  per scene.

Shapes: the smallest that reach every code path of the kernels -- one wave per row, 4 per block; lanes along j hold
MGAR_DAFM_MAX_N / 64 = 2 columns each; lanes along d step 256 floats (the table of fusion_cases.DAFM_CASES without the case
that is about E underflowing, which this mode does not compute)."""
import os

import numpy as np
import torch

CASES = {
    "n1_n64_n65_D64": dict(counts=[1, 64, 65, 2], D=64),           # n = 1; second column register starts; 16 lanes along d
    "n128_n127_D192": dict(counts=[128, 127, 3], D=192),           # full capacity; 258 rows (258 % 4 = 2); partial trip along d
    "empty_scenes_D320": dict(counts=[5, 0, 7, 0], D=320),         # duplicate offsets mid / end; partial second trip along d
    "large_logits": dict(counts=[33], D=512, qk_scale=4.0),        # large logits through __expf
}
PRIORS = ("none", "seeded", "masked")
MASK_VALUE = -1e4           # exp(MASK_VALUE + anything the cases reach) == 0 in fp32 and in float64
RTOL, ATOL = 1e-4, 1e-5     # tests/test_fusion_edges_gpu.py (BASELINE.json north_star)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fusion_variants.npz")
# tests/golden/make_reference_fusion_variants_golden.py
LAYER_RTOL, LAYER_ATOL = 1e-4, 1e-6     # tests/test_reference_blocks.py::test_dafm_layer_matches_reference
THRESHOLD_GAP = 1e-3
FUSIONS = ("sum", "Attention_normal", "Attention_max", "Attention_multi", "Attention_gaussian")
NET_COUNTS = ((5, 5, 5), (2, 7, 4))
# fixture name -> (class in model/gat_model.py, sigma, stored outputs)
LAYERS = {"plain": ("FusionAttention", 10, ("Rp", "Lp")), "fa3": ("FusionAttention3", 3., ("Rp", "Lp")),
          "fa2": ("FusionAttention2", 1., ("out",)), "gauss": ("FusionAttention_gaussian", 3, ("Rp", "Lp"))}


def inputs(counts, D, qk_scale=1.0, seed=11):
    """q, k, v (rows, D), the upstream gradient, fp32 on the CPU -- drawn like fusion_cases.dafm_inputs."""
    g = torch.Generator().manual_seed(seed)
    rows = sum(counts)
    q = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    k = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    v = torch.randn(rows, D, generator=g)
    grad = torch.randn(rows, D, generator=g)
    return q, k, v, grad


def prior(kind, counts, seed=12):
    """One (n, n) fp32 block per scene, or None.  'seeded': uniform in [-1, 1].  'masked': the seeded prior with MASK_VALUE
    on a random half of the off-diagonal entries (the diagonal stays, so no row is masked out whole)."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed)
    blocks = []
    for n in counts:
        p = torch.rand(n, n, generator=g) * 2 - 1
        if kind == "masked":
            hide = (torch.rand(n, n, generator=g) < 0.5) & ~torch.eye(n, dtype=torch.bool)
            p = torch.where(hide, torch.full_like(p, MASK_VALUE), p)
        blocks.append(p)
    return blocks


def flat(blocks):
    return torch.cat([b.reshape(-1) for b in blocks])


def attention_add_ref(q, k, v, p, scale):
    """One scene, in the dtype of its inputs (float64 for the reference): (out, att).  p: (n, n) or None."""
    logits = q @ k.T * scale
    if p is not None:
        logits = logits + p
    att = torch.softmax(logits, dim=1)
    return att @ v, att


def reference(q, k, v, blocks, counts, scale, grad):
    """float64 over all scenes: out, att (packed), dq, dk, dv."""
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    r0, outs, atts = 0, [], []
    for s, n in enumerate(counts):
        if n:
            p = None if blocks is None else blocks[s].double()
            o, a = attention_add_ref(qd[r0:r0 + n], kd[r0:r0 + n], vd[r0:r0 + n], p, scale)
            outs.append(o); atts.append(a.detach().reshape(-1))
        r0 += n
    out = torch.cat(outs)
    out.backward(grad.double())
    return out.detach(), torch.cat(atts), qd.grad, kd.grad, vd.grad


def threshold_gap(A, counts):
    """Smallest |A_theta - 0.5| over the valid off-diagonal entries of a padded (S, MNP, MNP) A_theta."""
    gap = np.inf
    for s, n in enumerate(counts):
        blk = np.asarray(A[s, :n, :n], np.float64)
        gap = min(gap, np.abs(blk[~np.eye(n, dtype=bool)] - 0.5).min())
    return float(gap)


def net_tag(fusion, counts, mode):
    return "net_%s_%s_%s" % (fusion, "".join(str(c) for c in counts), mode)
