"""Generates tests/golden/reference_fusion_table.npz by RUNNING THE REFERENCE'S OWN classes (imported the way
make_reference_golden.py imports them, with its stubs) for the rows of the paper's Table I that the packed route of
GAR_Fusion_Net3 serves through the multi-head attention kernel or with one modality absent:

    FUSION = crossAtt | catandAtt      (MODALITY Multi, FEAT_NORM True, FEATURE_DIM 1024, HIDDEN_DIM 512)
    MODALITY = RGB | LiDAR             (FEAT_NORM False -- the reference raises UnboundLocalError with it -- both dims 512)

Net level: GAR_Fusion_Net3 of each configuration on the gar_* inputs of reference_torch_blocks.npz (read, not stored again),
actor counts (5, 5, 5) and (2, 7, 4) set through person_id, eval and train mode (Dropout p = 0, no_grad -- see
make_reference_golden.py); all 16 outputs, and the running statistics of bn_rgb / bn_lidar after the train passes of the two
FEAT_NORM configurations.  Layer level: cross_attention_fusion (seed 4) on n = 9 rows of width 512.

Weights are NOT stored: both sides fill them with tests/golden/param_fill.py.  The case tables, key names and the
assertions (every output finite; no valid off-diagonal entry of A_theta within 1e-3 of 0.5, so a predicted group cannot
flip under rounding) are those of tests/scene_mha_cases.py; tests/test_scene_mha_cpu.py runs them again on the committed file.
Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_fusion_table_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_reference_golden import gar_cfg, import_reference  # noqa: E402
from param_fill import fill_deterministic  # noqa: E402
from scene_mha_cases import (CONFIGS, LAYER_FILL_SEED, LAYER_N, LAYER_SEED, NET_COUNTS, check_fixture,  # noqa: E402
                             net_tag as tag)


def person_ids(counts, mnp):
    pid = -torch.ones((len(counts), mnp), dtype=torch.long)
    for s, n in enumerate(counts):
        pid[s, :n] = torch.arange(n)
    return pid


def main():
    _, gat = import_reference()
    blocks = np.load(os.path.join(HERE, "reference_torch_blocks.npz"))
    rgb, lid, bboxes, b3 = (torch.from_numpy(blocks[k]) for k in ("gar_rgb", "gar_lidar", "gar_bboxes", "gar_bboxes3d"))
    out = {}
    for config, over in CONFIGS.items():
        cfg = gar_cfg()
        for key, value in over.items():
            cfg[key] = value
        for counts in NET_COUNTS:
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
                    out["%s_%02d" % (tag(config, counts, mode), i)] = r.detach().numpy()
                if mode == "train" and cfg.FEAT_NORM:
                    for bn in ("bn_rgb", "bn_lidar"):
                        out["%s_%s_mean" % (tag(config, counts, mode), bn)] = getattr(net, bn).running_mean.numpy().copy()
                        out["%s_%s_var" % (tag(config, counts, mode), bn)] = getattr(net, bn).running_var.numpy().copy()

    # --- layer: cross_attention_fusion at its one width, 512
    g = torch.Generator().manual_seed(LAYER_SEED)
    R = torch.randn((LAYER_N, 512), generator=g); L = torch.randn((LAYER_N, 512), generator=g)
    layer = fill_deterministic(gat.cross_attention_fusion(), seed=LAYER_FILL_SEED).eval()
    with torch.no_grad():
        out.update(layer_R=R.numpy(), layer_L=L.numpy(), layer_out=layer(R, L).numpy())

    print("smallest |A_theta - 0.5| over the valid off-diagonal entries: %.4f" % check_fixture(out))
    path = os.path.join(HERE, "reference_fusion_table.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
