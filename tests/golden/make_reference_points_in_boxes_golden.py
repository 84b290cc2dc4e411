"""Generates tests/golden/reference_points_in_boxes.npz by RUNNING THE REFERENCE'S OWN points_in_boxes_cpu
(pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp, built from the reference's file by oracle/build_ref.sh into
oracle/_ref/, where the reference tree is present) on the seeded boundary case of point_crop_cases.py.
Stored: the boxes, the SHA-256 of the points (the test regenerates them from the seed and checks they are the same) and
the (boxes, points) in/out decisions, packed 8 per byte along the points.
Run from the repo root after build():  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_points_in_boxes_golden.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from point_crop_cases import CASE, boundary_cases  # noqa: E402


def main():
    from oracle import oracle as O
    ref = O.load_reference_roiaware()
    if ref is None:
        raise SystemExit("oracle/_ref/roiaware_pool3d_ref.so is not built (oracle/build_ref.sh needs the reference tree)")
    boxes, pts = boundary_cases(*CASE)
    mask = torch.zeros((boxes.shape[0], pts.shape[0]), dtype=torch.int32)
    ref.points_in_boxes_cpu(torch.from_numpy(boxes), torch.from_numpy(pts), mask)
    m = mask.numpy()
    assert set(np.unique(m).tolist()) <= {0, 1}
    np.savez_compressed(os.path.join(HERE, "reference_points_in_boxes.npz"), boxes=boxes,
                        pts_sha256=np.array(hashlib.sha256(pts.tobytes()).hexdigest()),
                        mask_bits=np.packbits(m.astype(np.uint8), axis=1), n_pts=np.array(pts.shape[0]))
    print("points inside a box: %d of %d" % (m.sum(), m.size))


if __name__ == "__main__":
    main()
