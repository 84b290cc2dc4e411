"""Per-actor point crop: the oracle's box test is PINNED against the reference's own CPU
implementation -- points_in_boxes_cpu of the reference's pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:118-168, whose
decisions are stored in tests/golden/reference_points_in_boxes.npz (it is built from the reference's file by
oracle/build_ref.sh into the git-ignored oracle/_ref/ where that tree is present, and then run as well) -- on points
crowded around the box faces, where every rounding choice of the test (float vs double compares, cos / sin of the negated
heading, un-contracted products) shows.  The two differ only in MARGIN (1e-2 in the CPU function, 1e-5 in the CUDA
kernels roiaware_pool3d_kernel.cu:27 / roipoint_pool3d_kernel.cu:27), which the oracle takes as a parameter."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from point_crop_cases import CASE, boundary_cases  # noqa: E402

GOLD = os.path.join(HERE, "golden", "reference_points_in_boxes.npz")


def test_oracle_box_test_equals_the_reference_cpu_build(oracle):
    """Against the decisions of the reference's points_in_boxes_cpu stored in tests/golden/reference_points_in_boxes.npz
    (make_reference_points_in_boxes_golden.py); where oracle/_ref holds the reference's build it is run as well."""
    g = np.load(GOLD)
    boxes, pts = boundary_cases(*CASE)
    assert np.array_equal(boxes, g["boxes"]) and hashlib.sha256(pts.tobytes()).hexdigest() == str(g["pts_sha256"]), \
        "the seeded boundary case no longer reproduces the fixture's inputs"
    want = np.unpackbits(g["mask_bits"], axis=1, count=int(g["n_pts"])).astype(np.int32)
    ref = oracle.load_reference_roiaware()
    if ref is not None:
        live = torch.zeros((boxes.shape[0], pts.shape[0]), dtype=torch.int32)
        ref.points_in_boxes_cpu(torch.from_numpy(boxes), torch.from_numpy(pts), live)
        assert np.array_equal(live.numpy(), want), "the reference's build disagrees with the stored fixture"
    got = oracle.points_in_boxes_mask(boxes, pts, 1e-2)
    assert np.array_equal(got, want), "%d of %d decisions differ" % ((got != want).sum(), got.size)
    inside = want.sum()
    assert 0.2 * pts.shape[0] < inside < 0.95 * pts.shape[0]          # the cases straddle the faces
    # the margin matters on these points: the CUDA kernels' 1e-5 gives a different answer for thousands of them
    assert (oracle.points_in_boxes_mask(boxes, pts, 1e-5) != got).sum() > 1000


def test_oracle_points_in_boxes_and_roipoint_pool_semantics(oracle):
    """First box wins; -1 background; crop = first S inside points in index order, cyclic duplication, empty flag."""
    boxes = np.array([[[0, 0, 0, 2, 2, 2, 0.0], [0.5, 0, 0, 2, 2, 2, 0.0], [50, 50, 0, 1, 1, 1, 0.3]]], np.float32)
    pts = np.array([[[0.2, 0, 0], [1.4, 0, 0], [9, 9, 9], [-0.9, 0.9, -0.9], [0, 0, 1.0001]]], np.float32)
    assert oracle.points_in_boxes(boxes, pts).tolist() == [[0, 1, -1, 0, -1]]
    feat = np.arange(5 * 2, dtype=np.float32).reshape(1, 5, 2)
    pooled, empty = oracle.roipoint_pool3d(pts, boxes, feat, 4)
    assert empty.tolist() == [[0, 0, 1]]
    assert pooled[0, 0, :, 0].tolist() == pytest.approx([0.2, -0.9, 0.2, -0.9])        # points 0 and 3, duplicated cyclically
    assert pooled[0, 0, :, 3:].tolist() == [[0, 1], [6, 7], [0, 1], [6, 7]]
    assert pooled[0, 1, :, 0].tolist() == pytest.approx([0.2, 1.4, 0.2, 1.4])
    assert not pooled[0, 2].any()
