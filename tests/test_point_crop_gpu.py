"""Per-actor point crop on the device (csrc/point_crop.hip) against the C oracle, whose box test is pinned to the
reference's own CPU build (tests/test_point_crop_cpu.py): points_in_boxes_gpu and RoIPointPool3d through the mirrored
reference modules (pcdet/ops/roiaware_pool3d, pcdet/ops/roipoint_pool3d), bit-exact."""
import numpy as np
import pytest
import torch

from test_point_crop_cpu import boundary_cases as _boundary_cases  # tests/golden/point_crop_cases.py

pytestmark = pytest.mark.gpu


def test_points_in_boxes_gpu_vs_oracle(oracle):
    from multimodal_gar_amd.pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils import points_in_boxes_gpu
    boxes, pts = _boundary_cases(5, 32, 64000)                      # crowded around the faces of overlapping boxes
    boxes = np.stack([boxes, boxes[::-1]])                          # two samples, different box order
    pts = np.stack([pts, pts[::-1]])
    got = points_in_boxes_gpu(torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(boxes.copy()).cuda())
    want = oracle.points_in_boxes(boxes, pts)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert (want >= 0).mean() > 0.2 and (want < 0).mean() > 0.02


@pytest.mark.parametrize("n_pts,n_boxes,c,s", [(16384, 32, 128, 512), (4096, 7, 3, 64), (1000, 3, 0, 2048)])
def test_roipoint_pool3d_vs_oracle(oracle, n_pts, n_boxes, c, s):
    from multimodal_gar_amd import synthetic as S
    from multimodal_gar_amd.pcdet.ops.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    sc = S.scene_batch(9, 2, n_boxes, n_pts)
    xyz = np.ascontiguousarray(sc["points"][:, :, :3])
    boxes = sc["bboxes3d"][:, :n_boxes].copy()
    boxes[1, -1, :3] = 500.0                                         # one box far from every point: empty
    rng = np.random.default_rng(3)
    feat = rng.standard_normal((2, n_pts, c)).astype(np.float32)
    pool = RoIPointPool3d(num_sampled_points=s, pool_extra_width=[0.2, 0.1, 0.0])
    pooled, empty = pool(torch.from_numpy(xyz).cuda(), torch.from_numpy(feat).cuda(), torch.from_numpy(boxes).cuda())
    big = boxes.copy()
    big[..., 3:6] += np.array([0.2, 0.1, 0.0], np.float32)
    want_p, want_e = oracle.roipoint_pool3d(xyz, big, feat, s)
    assert pooled.shape == (2, n_boxes, s, 3 + c) and empty.dtype == torch.int32
    assert np.array_equal(empty.cpu().numpy(), want_e) and want_e[1, -1] == 1 and want_e.sum() < want_e.size
    assert np.array_equal(pooled.cpu().numpy(), want_p)
    counts = [(want_p[0, m, :, :3] != want_p[0, m, 0, :3]).any() for m in range(n_boxes)]
    assert any(counts)                                               # at least one box with more than one distinct point
