"""Generates tests/golden/reference_fusion_variants.npz by RUNNING THE REFERENCE'S OWN classes (imported the way
make_reference_golden.py imports them, with its stubs) for the fusion configurations that the packed route of
GAR_Fusion_Net3 serves besides the shipped one:

    FUSION = sum | Attention_normal | Attention_max | Attention_multi | Attention_gaussian

Net level: GAR_Fusion_Net3 of each configuration on the gar_* inputs of reference_torch_blocks.npz (read, not stored again),
actor counts (5, 5, 5) and (2, 7, 4) set through person_id, eval and train mode (Dropout p = 0, no_grad -- see
make_reference_golden.py); all 16 outputs, and the running statistics of bn_rgb / bn_lidar after the train pass.
Layer level (width 64, n = 9): (R', L') of FusionAttention, FusionAttention3(sigma=3), FusionAttention_gaussian(sigma=3) and
the output of FusionAttention2(sigma=1).

Weights are NOT stored: both sides fill them with tests/golden/param_fill.py.  The file is about 260 KB (376 float32
arrays, compressed): 20 net runs x 16 outputs, the (512,) running statistics of the 10 train runs, and the layer block.
The case tables, key names and the threshold measure are those of tests/dafm_prior_cases.py, which the tests read too.

Asserted here, and again on the committed file by tests/test_dafm_prior_cpu.py:
  * every output is finite;
  * no valid off-diagonal entry of A_theta lies within 1e-3 of 0.5 (a predicted group cannot flip under rounding);
  * every prior-carrying layer's output differs from the same layer under a zero prior by more than 100 x the tolerance the
    layer tests use (LAYER_RTOL of the largest entry + LAYER_ATOL): a kernel that dropped the prior could not pass.  The
    zero-prior outputs are stored as `layer_<name>_noprior_*` for that check.
Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_fusion_variants_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_reference_golden import gar_cfg, import_reference, t64  # noqa: E402
from oracle import oracle as O  # noqa: E402
from param_fill import fill_deterministic  # noqa: E402
from dafm_prior_cases import (FUSIONS, LAYER_ATOL, LAYER_RTOL, LAYERS, NET_COUNTS as COUNTS, THRESHOLD_GAP,  # noqa: E402
                              net_tag as tag, threshold_gap)


def person_ids(counts, mnp):
    pid = -torch.ones((len(counts), mnp), dtype=torch.long)
    for s, n in enumerate(counts):
        pid[s, :n] = torch.arange(n)
    return pid


def prior_margin(out, out_noprior):
    """(difference to the zero-prior output) / (100 x the layer tolerance): must exceed 1."""
    out, out_noprior = np.asarray(out, np.float64), np.asarray(out_noprior, np.float64)
    return float(np.abs(out - out_noprior).max() / (100 * (LAYER_RTOL * np.abs(out).max() + LAYER_ATOL)))


def main():
    _, gat = import_reference()
    blocks = np.load(os.path.join(HERE, "reference_torch_blocks.npz"))
    rgb, lid, bboxes, b3 = (torch.from_numpy(blocks[k]) for k in ("gar_rgb", "gar_lidar", "gar_bboxes", "gar_bboxes3d"))
    out = {}
    gaps = []
    for fusion in FUSIONS:
        cfg = gar_cfg()
        cfg.FUSION = fusion
        for counts in COUNTS:
            pid = person_ids(counts, rgb.shape[1])
            for mode in ("eval", "train"):
                net = fill_deterministic(gat.GAR_Fusion_Net3(cfg), seed=5)
                net.train(mode == "train")
                for mod in net.modules():
                    if isinstance(mod, torch.nn.Dropout):
                        mod.p = 0.0
                with torch.no_grad():
                    res = net(rgb, lid, bboxes, b3, None, pid)
                assert len(res) == 16
                for i, r in enumerate(res):
                    assert torch.isfinite(r).all(), (fusion, counts, mode, i)
                    out["%s_%02d" % (tag(fusion, counts, mode), i)] = r.detach().numpy()
                gap = threshold_gap(res[0].detach().numpy(), counts)
                assert gap > THRESHOLD_GAP, (fusion, counts, mode, gap)
                gaps.append(gap)
                if mode == "train":
                    for bn in ("bn_rgb", "bn_lidar"):
                        out["%s_%s_mean" % (tag(fusion, counts, mode), bn)] = getattr(net, bn).running_mean.numpy().copy()
                        out["%s_%s_var" % (tag(fusion, counts, mode), bn)] = getattr(net, bn).running_var.numpy().copy()
    print("smallest |A_theta - 0.5| over the valid off-diagonal entries: %.4f" % min(gaps))

    # --- layers (reduced width 64), inputs drawn like the dafm_* block of make_reference_golden.py, plus GIoU of seeded boxes
    g = torch.Generator().manual_seed(4321)
    n = 9
    R = torch.randn((n, 64), generator=g); L = torch.randn((n, 64), generator=g)
    ctr = torch.rand((n, 3), generator=g) * 20
    De = torch.cdist(ctr, ctr); De.fill_diagonal_(0)
    xy = torch.rand((n, 2), generator=g) * 300; wh = torch.rand((n, 2), generator=g) * 200 + 20
    Dg = t64(O.generalized_box_iou)(torch.cat([xy, xy + wh], -1), torch.cat([xy, xy + wh], -1))
    out.update(layer_R=R.numpy(), layer_L=L.numpy(), layer_De=De.numpy(), layer_Dg=Dg.numpy())
    far, zero = torch.full((n, n), 1e4), torch.zeros(n, n)      # exp(-far^2 / .) == 0 in fp32: a zero prior on both branches
    for name, (cls, sigma, _) in LAYERS.items():
        layer = fill_deterministic(getattr(gat, cls)(input_dim=64, out_dim=64, sigma=sigma), seed=4).eval()
        with torch.no_grad():
            res, res0 = layer(R, L, Dg, De), layer(R, L, zero, far)
        parts = [("out", res, res0)] if cls == "FusionAttention2" else list(zip(("Rp", "Lp"), res, res0))
        for suffix, r, r0 in parts:
            assert torch.isfinite(r).all(), (name, suffix)
            out["layer_%s_%s" % (name, suffix)] = r.numpy()
            if name != "plain":
                margin = prior_margin(r.numpy(), r0.numpy())
                print("layer %s %s: prior moves the output by %.1f x (100 x tolerance)" % (name, suffix, margin))
                assert margin > 1, (name, suffix, margin)
                out["layer_%s_noprior_%s" % (name, suffix)] = r0.numpy()
            else:
                assert torch.equal(r, r0)

    path = os.path.join(HERE, "reference_fusion_variants.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
