"""RoI-grid lift of the valid boxes only (batch_dict['roi_counts']): PointGridRoIHead and VoxelRCNNHead with counts
[3, 0, 5] -- an empty sample in the middle -- against the pooling layers called directly on hand-built compacted grid points
(train mode, bit for bit) and against the valid rows of the padded run (eval mode, where queries are independent)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS, N_BOX = [3, 0, 5], 5
VALID = [b * N_BOX + i for b, c in enumerate(COUNTS) for i in range(c)]


def _scene(seed, n_points):
    from multimodal_gar_amd import synthetic as S
    sc = S.scene_batch(seed, len(COUNTS), N_BOX, n_points)
    return torch.from_numpy(np.ascontiguousarray(sc["points"])), torch.from_numpy(sc["bboxes3d"])[:, :N_BOX, :].contiguous()


def _point_grid(train):
    from multimodal_gar_amd import workload as W
    from multimodal_gar_amd.pcdet.models.roi_heads.point_grid_head import PointGridRoIHead
    f, p, c = len(COUNTS), 1024, 16
    points, b3 = _scene(11, p)
    head = fill_deterministic(PointGridRoIHead(c, W.lidar_model_cfg(p)["ROI_HEAD"]), seed=5).train(train).cuda()
    feats = torch.randn(f * p, c, generator=torch.Generator().manual_seed(4)).cuda()
    bidx = torch.arange(f, dtype=torch.float32).view(f, 1, 1).expand(f, p, 1)
    coords = torch.cat([bidx, points[..., :3]], -1).view(f * p, 4).cuda()

    def data(**extra):
        return dict(batch_size=f, gt_boxes=b3.cuda(), point_coords=coords, point_features=feats,
                    point_batch_cnt=torch.full((f,), p, dtype=torch.int32, device="cuda"), **extra)
    return head, data, coords, feats, b3.cuda()


def test_point_grid_head_train_equals_the_layer_on_compacted_grid_points():
    from multimodal_gar_amd.pcdet.models.roi_heads.voxelrcnn_head import global_grid_points_of_roi
    head, data, coords, feats, b3 = _point_grid(True)
    g = head.grid_size
    with torch.no_grad():
        got = copy.deepcopy(head)(data(roi_counts=COUNTS))["pooled_features"]
        grid, _ = global_grid_points_of_roi(b3.view(-1, 7)[VALID], g)
        cnt = torch.tensor([c * g ** 3 for c in COUNTS], dtype=torch.int32, device="cuda")
        _, want = copy.deepcopy(head).roi_grid_pool_layer(
            xyz=coords[:, 1:4].contiguous(), xyz_batch_cnt=torch.full((3,), 1024, dtype=torch.int32, device="cuda"),
            new_xyz=grid.view(-1, 3).contiguous(), new_xyz_batch_cnt=cnt, features=feats)
    assert got.shape[0] == 8 and got.shape[1] == g ** 3
    assert torch.equal(got, want.reshape(got.shape)) and got.abs().sum() > 0


def test_point_grid_head_eval_compacted_rows_are_the_valid_rows_and_no_key_is_unchanged():
    from multimodal_gar_amd.pcdet.models.roi_heads.voxelrcnn_head import global_grid_points_of_roi
    head, data, coords, feats, b3 = _point_grid(False)
    g = head.grid_size
    with torch.no_grad():
        padded = head(data())["pooled_features"]
        got = head(data(roi_counts=COUNTS))["pooled_features"]
        grid, _ = global_grid_points_of_roi(b3, g)      # no roi_counts: the layer on every box, as before
        _, want = head.roi_grid_pool_layer(
            xyz=coords[:, 1:4].contiguous(), xyz_batch_cnt=torch.full((3,), 1024, dtype=torch.int32, device="cuda"),
            new_xyz=grid.view(-1, 3).contiguous(),
            new_xyz_batch_cnt=torch.full((3,), N_BOX * g ** 3, dtype=torch.int32, device="cuda"), features=feats)
    assert padded.shape[0] == 15 and torch.equal(padded, want.reshape(padded.shape))
    assert got.shape[0] == 8 and torch.equal(got, padded[VALID])


def _voxel_net(train):
    from multimodal_gar_amd import workload as W
    from multimodal_gar_amd.pcdet.models import build_network
    ds = W.SyntheticDataset()
    pts, b3 = _scene(3, 4096)
    net = fill_deterministic(build_network(W.lidar_model_cfg(4096, "voxel"), 1, ds), seed=9).train(train).cuda()

    def data(**extra):
        d = W.voxelize_batch(pts.cuda(), ds)
        d["gt_boxes"] = b3.cuda()
        d.update(extra)
        return d
    return net, data, b3.cuda()


def test_voxel_rcnn_head_eval_compacted_rows_are_the_valid_rows():
    net, data, _ = _voxel_net(False)
    with torch.no_grad():
        padded = net(data())
        got = net(data(roi_counts=COUNTS))
    assert padded["pooled_features"].shape[0] == 15 and got["pooled_features"].shape[0] == 8
    assert torch.equal(got["pooled_features"], padded["pooled_features"][VALID]) and got["pooled_features"].abs().sum() > 0
    assert got["shared_feature"].shape[0] == 8


def _voxel_layers_directly(head, out, boxes, counts):
    """The head's pooling layers called on hand-built grid points of `boxes` (rows, 7), counts[b] of them in sample b."""
    from multimodal_gar_amd.pcdet.models.roi_heads.voxelrcnn_head import global_grid_points_of_roi
    from multimodal_gar_amd.pcdet.utils import common_utils
    g = head.pool_cfg.GRID_SIZE
    grid, _ = global_grid_points_of_roi(boxes, g)
    grid = grid.view(-1, 3)
    lo, vs = head.point_cloud_range, head.voxel_size
    vox = torch.cat([(grid[:, i:i + 1] - lo[i]) // vs[i] for i in range(3)], dim=-1)
    bidx = torch.tensor([b for b, c in enumerate(counts) for _ in range(c * g ** 3)], device="cuda", dtype=grid.dtype).view(-1, 1)
    cnt = torch.tensor([c * g ** 3 for c in counts], dtype=torch.int32, device="cuda")
    want = []
    for k, src in enumerate(head.pool_cfg.FEATURES_SOURCE):
        stride = out['multi_scale_3d_strides'][src]
        sp = out['multi_scale_3d_features'][src]
        centres = common_utils.get_voxel_centers(sp.indices[:, 1:4], downsample_times=stride, voxel_size=vs, point_cloud_range=lo)
        feat = head.roi_grid_pool_layers[k](
            xyz=centres.contiguous(), xyz_batch_cnt=torch.bincount(sp.indices[:, 0].long(), minlength=len(counts)).int(),
            new_xyz=grid.contiguous(), new_xyz_batch_cnt=cnt, new_coords=torch.cat([bidx, vox // stride], -1).int().contiguous(),
            features=sp.features.contiguous(), voxel2point_indices=common_utils.generate_voxel2pinds(sp))
        want.append(feat.view(-1, g ** 3, feat.shape[-1]))
    return torch.cat(want, -1)


def test_voxel_rcnn_head_train_equals_the_layers_on_compacted_grid_points():
    net, data, b3 = _voxel_net(True)
    with torch.no_grad():
        out = net(data(roi_counts=COUNTS))               # leaves the trunk's multi-scale features in the dict
        got = copy.deepcopy(net.roi_head).roi_grid_pool(out)
        want = _voxel_layers_directly(copy.deepcopy(net.roi_head), out, b3.view(-1, 7)[VALID], COUNTS)
    assert got.shape[0] == 8 and torch.equal(got, want) and got.abs().sum() > 0


@pytest.mark.parametrize("train", [False, True])
def test_voxel_rcnn_head_without_the_key_is_unchanged(train):
    """No roi_counts: every box of every sample, bit for bit what the layers give on the full grid."""
    net, data, b3 = _voxel_net(train)
    with torch.no_grad():
        out = net(data())
        got = copy.deepcopy(net.roi_head).roi_grid_pool(out)
        want = _voxel_layers_directly(copy.deepcopy(net.roi_head), out, b3.view(-1, 7), [N_BOX] * len(COUNTS))
    assert got.shape[0] == 15 and torch.equal(got, want) and got.abs().sum() > 0
    if not train:
        assert torch.equal(out["pooled_features"], got)
