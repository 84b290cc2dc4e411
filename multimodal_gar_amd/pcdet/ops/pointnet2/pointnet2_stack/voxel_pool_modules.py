"""Voxel RoI pooling layer.

Mirror of the reference's pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py
(NeighborVoxelSAModuleMSG): same constructor keywords and sub-module names (groupers,
mlps_in, mlps_pos, mlps_out).
"""
import os
from typing import List

import torch
import torch.nn as nn

from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import pointnet2_stack_cuda as pointnet2
from . import voxel_query_utils
from .....eval_route import bn_frozen, cached, hooked, needs_grad
from .....nn_utils import PointwiseSequential, _is_pointwise


class _FusedVoxelRoIPool(Function):
    """pooled (C, M) = max_s relu(feats[idx[m, s]] + BN_pos(w_pos . rel_xyz)) on csrc/voxel_roi_pool.hip: everything
    between mlps_in and mlps_out of one scale (reference voxel_pool_modules.py:94-117) without any (C, M, nsample) tensor."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, feats, idx_raw, w_pos, gamma, beta, bn):
        n_query, nsample = idx_raw.shape
        chans = feats.shape[1]
        xyz, new_xyz, feats = xyz.contiguous(), new_xyz.contiguous(), feats.contiguous()
        w_pos, gamma, beta = w_pos.contiguous().float(), gamma.float(), beta.float()
        dev = xyz.device
        train_stats = bn.training or not bn.track_running_stats
        moments = None
        if train_stats:
            mean = torch.empty((chans,), dtype=torch.float32, device=dev)
            invstd = torch.empty_like(mean)
            moments = torch.empty((10,), dtype=torch.float64, device=dev)
            track = bn.track_running_stats and bn.running_mean is not None
            pointnet2.voxel_roi_pool_stats(n_query, nsample, chans, xyz, new_xyz, idx_raw, w_pos, bn.eps,
                                           bn.momentum if bn.momentum is not None else 0.1, moments, mean, invstd,
                                           bn.running_mean if track else None, bn.running_var if track else None,
                                           bn.num_batches_tracked if track else None)
        else:
            mean, invstd = bn.running_mean.float(), torch.rsqrt(bn.running_var.float() + bn.eps)
        pooled = torch.empty((chans, n_query), dtype=feats.dtype, device=dev)
        arg = torch.empty((chans, n_query), dtype=torch.uint8, device=dev)
        pointnet2.voxel_roi_pool_fwd(n_query, nsample, chans, xyz, new_xyz, feats, idx_raw, w_pos, mean, invstd, gamma, beta, pooled, arg)
        ctx.save_for_backward(xyz, new_xyz, idx_raw, w_pos, mean, invstd, gamma, moments, pooled, arg)
        ctx.meta = (feats.shape, train_stats)
        ctx.mark_non_differentiable(arg)
        return pooled, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, dpooled, darg=None):
        xyz, new_xyz, idx_raw, w_pos, mean, invstd, gamma, moments, pooled, arg = ctx.saved_tensors
        (n_rows, chans), train_stats = ctx.meta
        n_query, nsample = idx_raw.shape
        dfeats = torch.zeros((n_rows, chans), dtype=torch.float32, device=xyz.device) if ctx.needs_input_grad[2] else None
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        dw = torch.empty_like(w_pos)
        pointnet2.voxel_roi_pool_bwd(n_query, nsample, chans, xyz, new_xyz, idx_raw, w_pos, mean, invstd, gamma, moments, train_stats,
                                     dpooled.contiguous().float(), pooled.float(), arg, dfeats, dgamma, dbeta, dw)
        return None, None, dfeats, None, dw, dgamma, dbeta, None


class _RowsLinear(Function):
    """z = x W^T for row-major x (N, C_in) with N in the millions and W (C_out, C_in) tiny.  Forward and dX are plain GEMMs; the
    weight gradient dz^T x -- a (C_out x C_in) result reduced over N rows, which the library runs at 2-3 TFLOP/s (4.3 ms at
    N = 4.15 M, C 32) -- goes to csrc/rowmajor_dw.hip (both operands streamed once through the MFMA)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        dz = dz.contiguous()
        dx = dz @ w if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = pointnet2.rowmajor_dw(dz, x) if (x.is_cuda and w.shape[0] <= 96 and w.shape[1] <= 128) else dz.t() @ x
        return dx, dw


# Inference (every BatchNorm of a scale not training, no gradient required): mlps_in folds into one GEMM with bias on the voxel
# rows as they are, and pooling + mlps_out run as ONE kernel that writes its columns of the caller's row-major buffer
# (mgar_voxel_roi_pool_eval_fwd / mgar_voxel_roi_pool_eval_bf16_fwd, csrc/voxel_roi_pool.hip).  MGAR_VRP_EVAL_FUSE=0 (or this flag) restores the train-mode
# kernels' path around torch's batch norm (A/B in tests and profiles).
MGAR_VRP_EVAL_FUSE = os.environ.get("MGAR_VRP_EVAL_FUSE", "1") != "0"
_EVAL_MAXC = 32     # channels = lanes of a half-wave, on both sides of mlps_out


def _conv_bn(seq, conv_type, bn_type, n_allowed):
    """(conv, bn) of a [point-wise conv, BatchNorm(, ReLU)] container, or None"""
    mods = list(seq)
    if len(mods) not in n_allowed or not (isinstance(mods[0], conv_type) and _is_pointwise(mods[0]) and isinstance(mods[1], bn_type)):
        return None
    if len(mods) == 3 and not isinstance(mods[2], nn.ReLU):
        return None
    return mods[0], mods[1]


def eval_fuse_plan(module, k, features, xyz):
    """Whether scale k of a NeighborVoxelSAModuleMSG runs on the inference route (NeighborVoxelSAModuleMSG._eval_scale):
    -> (conv_in, bn_in, pos_conv, pos_bn, conv_out, bn_out, relu), or None for today's path.  Fused when the switch
    (MGAR_VRP_EVAL_FUSE) is on, module.fused is set and it pools with max_pool, the features are 2-D fp32 or bf16 rows on the
    device (as are the voxel centres), mlps_in[k] is [point-wise Conv1d, BatchNorm1d], mlps_pos[k] [point-wise Conv2d(3 -> C),
    BatchNorm2d], mlps_out[k] [point-wise Conv1d, BatchNorm1d(, ReLU)], none of the three BatchNorms is training and each has
    running statistics, C and C_out <= 32, and no gradient is required: grad mode is off, or neither the features nor a
    parameter of these modules requires one.  A forward (pre-)hook on any of these modules or their containers keeps the scale
    unfused, so the hook still sees its module run.  Reads nothing but attributes: no device work, no synchronisation."""
    if not (MGAR_VRP_EVAL_FUSE and module.fused and module.pool_method == 'max_pool'):
        return None
    if not (features.is_cuda and xyz.is_cuda and features.ndim == 2 and features.dtype in (torch.float32, torch.bfloat16)):
        return None
    seqs = (module.mlps_in[k], module.mlps_pos[k], module.mlps_out[k])
    pairs = (_conv_bn(seqs[0], nn.Conv1d, nn.BatchNorm1d, (2,)), _conv_bn(seqs[1], nn.Conv2d, nn.BatchNorm2d, (2,)),
             _conv_bn(seqs[2], nn.Conv1d, nn.BatchNorm1d, (2, 3)))
    if None in pairs:
        return None
    (conv_in, bn_in), (pos_conv, pos_bn), (conv_out, bn_out) = pairs
    chans = conv_in.out_channels
    if not (pos_conv.in_channels == 3 and pos_conv.out_channels == chans and conv_out.in_channels == chans
            and conv_in.in_channels == features.shape[1] and chans <= _EVAL_MAXC and conv_out.out_channels <= _EVAL_MAXC):
        return None
    if not all(bn_frozen(bn) for bn in (bn_in, pos_bn, bn_out)):
        return None
    mods = [m for seq in seqs for m in seq]
    if needs_grad(features, (p for m in mods for p in m.parameters())):
        return None
    if hooked(*mods, *seqs, module.relu):
        return None
    return conv_in, bn_in, pos_conv, pos_bn, conv_out, bn_out, len(seqs[2]) == 3


def folded_mlp_in(conv, bn):
    """mlps_in = point-wise Conv1d + eval-mode BatchNorm1d as one GEMM with bias on rows: -> {dtype: (W', b)} for float32 and
    bfloat16 rows, feats_in = features W'^T + b.  (s, b) = sparse_ops.fold_bn(bn, conv.bias); W' = s[:, None] * W formed in float64
    and rounded once to fp32; the bf16 pair is that pair rounded once more (operands and bias of a bf16 GEMM).  Cached on the
    convolution (eval_route.cached) under the weight, derived from fold_bn's own cached pair: an in-place update of any tensor
    read recomputes, a second forward launches nothing."""
    from .....sparse_ops import fold_bn
    scale, shift = fold_bn(bn, conv.bias)

    def build():
        w = conv.weight.detach().view(conv.out_channels, conv.in_channels).double()
        w = (scale.double()[:, None] * w).float().contiguous()
        return {torch.float32: (w, shift), torch.bfloat16: (w.to(torch.bfloat16), shift.to(torch.bfloat16))}
    return cached(conv, "_mgar_folded_in", (conv.weight,), build, derived_from=(scale, shift))


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges: List[List[int]], radii: List[float],
                 nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True, pool_method='max_pool'):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for max_range, nsample, radius, spec in zip(query_ranges, nsamples, radii, mlps):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(max_range, radius, nsample))
            self.mlps_in.append(PointwiseSequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False),
                                              nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(PointwiseSequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False),
                                               nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(PointwiseSequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False),
                                               nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self.fused = True      # device path: csrc/voxel_roi_pool.hip (set False to run the un-fused op chain on the device)
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def _mlp_in_rows(self, k, features):
        """mlps_in[k] = Conv1d(1x1, no bias) + BatchNorm1d on ALL voxels (reference voxel_pool_modules.py:86-88), evaluated on
        the row-major (N, C) features as they are: one GEMM + the row-major BatchNorm kernels (csrc/channels_last.hpp), without
        the two transposing copies of the (1, C, N) formulation (7.6 + 6 ms per step at config c3).  Device + train mode only: a
        scale whose BatchNorms are all in eval mode takes the inference route instead (eval_fuse_plan, _eval_scale).
        bf16 rows (the bf16 trunk, forward only): one bf16 GEMM, then the bf16 row-major BatchNorm -- the (N, C) bf16 result is what
        mgar_voxel_roi_pool_fwd_bf16 reads."""
        conv, bn = self.mlps_in[k][0], self.mlps_in[k][1]
        if not (features.is_cuda and bn.training and conv.bias is None and len(self.mlps_in[k]) == 2):
            return None
        from .....bn_ops import bn_act_rows
        w = conv.weight.view(conv.out_channels, conv.in_channels)
        if features.dtype == torch.bfloat16:
            if needs_grad(features, (w,)):
                return None
            return bn_act_rows(features.contiguous() @ w.detach().to(torch.bfloat16).t(), bn, False)
        if features.dtype != torch.float32:
            return None
        z = _RowsLinear.apply(features.contiguous(), w)   # (N, C)
        return bn_act_rows(z, bn, False) if z.dtype == torch.float32 else None   # under autocast z is bf16: the caller's formulation

    def _eval_scale(self, k, plan, xyz, new_xyz, new_coords, features, voxel2point_indices, out):
        """Scale k on the inference route into out (M, C_out), rows of the features' dtype or a column slice of a wider buffer:
        one GEMM with bias for mlps_in on all voxels, the voxel query, one kernel for everything behind it.  Autocast is
        switched off inside: the precision is the features' own."""
        conv_in, bn_in, pos_conv, pos_bn, conv_out, bn_out, relu = plan
        from .....sparse_ops import fold_bn
        grouper = self.groupers[k]
        chans, c_out = conv_in.out_channels, conv_out.out_channels
        with torch.no_grad(), torch.autocast(device_type=features.device.type, enabled=False):
            w_in, b_in = folded_mlp_in(conv_in, bn_in)[features.dtype]
            feats_in = torch.addmm(b_in, features.detach(), w_in.t())                                # (N, C)
            idx_raw = voxel_query_utils.voxel_query_raw(grouper.max_range, grouper.radius, grouper.nsample, xyz, new_xyz,
                                                        new_coords, voxel2point_indices)
            pos_scale, pos_shift = fold_bn(pos_bn, pos_conv.bias)
            out_scale, out_shift = fold_bn(bn_out, conv_out.bias)
            pointnet2.voxel_roi_pool_eval_fwd(idx_raw.shape[0], idx_raw.shape[1], chans, c_out, xyz.contiguous(), new_xyz.contiguous(),
                                              feats_in, idx_raw, pos_conv.weight.detach().view(chans, 3).float().contiguous(),
                                              pos_scale, pos_shift, conv_out.weight.detach().view(c_out, chans).float().contiguous(),
                                              out_scale, out_shift, relu, out)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, out=None):
        """xyz (N, 3) voxel centres, features (N, C_in), new_xyz (M, 3) grid points,
        new_coords (M, 4) [b, x, y, z] -> (M, sum_k mlps[k][-1]).
        out: optional (M, sum_k mlps[k][-1]) row-major result buffer of the features' dtype, or a column slice of a wider one;
        every scale on the inference route (eval_fuse_plan) writes its columns there directly, and without `out` the module
        allocates the buffer itself -- no torch.cat either way.
        Reference: voxel_pool_modules.py:70-130."""
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()  # -> [b, z, y, x]
        plans = [eval_fuse_plan(self, k, features, xyz) for k in range(len(self.groupers))]
        if plans and all(p is not None for p in plans):
            widths = [p[4].out_channels for p in plans]
            if out is None:
                out = torch.empty((new_xyz.shape[0], sum(widths)), dtype=features.dtype, device=features.device)
            elif tuple(out.shape) != (new_xyz.shape[0], sum(widths)) or out.dtype != features.dtype:
                raise ValueError("NeighborVoxelSAModuleMSG: out must be (%d, %d) of %s" % (new_xyz.shape[0], sum(widths), features.dtype))
            col = 0
            for k, plan in enumerate(plans):
                self._eval_scale(k, plan, xyz, new_xyz, new_coords, features, voxel2point_indices, out[:, col:col + widths[k]])
                col += widths[k]
            return out
        result = self._forward_scales(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, plans)
        if out is None:
            return result
        out.copy_(result)
        return out

    def _forward_scales(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices, plans):
        per_scale = []
        for k, grouper in enumerate(self.groupers):
            if plans[k] is not None:       # some but not all scales on the inference route: its own (M, C_out), joined below
                part = torch.empty((new_xyz.shape[0], plans[k][4].out_channels), dtype=features.dtype, device=features.device)
                self._eval_scale(k, plans[k], xyz, new_xyz, new_coords, features, voxel2point_indices, part)
                per_scale.append(part)
                continue
            feats_in = self._mlp_in_rows(k, features)
            if feats_in is None:
                feats_in = self.mlps_in[k](features.permute(1, 0).unsqueeze(0))    # (1, C, N)
                feats_in = feats_in.squeeze(0).permute(1, 0).contiguous()          # (N, C)
            pos_conv, pos_bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
            if (self.fused and xyz.is_cuda and self.pool_method == 'max_pool' and feats_in.shape[1] <= 32 and pos_conv.bias is None
                    and not (torch.is_grad_enabled() and feats_in.dtype != torch.float32)):
                # device path: voxel query, then ONE kernel for group + position MLP + BatchNorm + ReLU + max
                # (csrc/voxel_roi_pool.hip); the CPU run below is the reference's op chain
                idx_raw = voxel_query_utils.voxel_query_raw(grouper.max_range, grouper.radius, grouper.nsample, xyz, new_xyz,
                                                            new_coords, voxel2point_indices)
                gamma = pos_bn.weight if pos_bn.affine else torch.ones(feats_in.shape[1], device=xyz.device)
                beta = pos_bn.bias if pos_bn.affine else torch.zeros(feats_in.shape[1], device=xyz.device)
                pooled, _ = _FusedVoxelRoIPool.apply(xyz, new_xyz, feats_in, idx_raw, pos_conv.weight.view(feats_in.shape[1], 3),
                                                     gamma, beta, pos_bn)                     # (C, M) channel-major
                per_scale.append(self.mlps_out[k](pooled.unsqueeze(0)).squeeze(0).permute(1, 0))
                continue
            grouped, grouped_xyz, empty = grouper(new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt,
                                                  feats_in, voxel2point_indices)
            keep = (~empty).view(-1, 1, 1).to(grouped.dtype)
            grouped = (grouped * keep).permute(1, 0, 2).unsqueeze(0)               # (1, C, M, nsample)
            rel_xyz = ((grouped_xyz - new_xyz.unsqueeze(-1)) * keep).permute(1, 0, 2).unsqueeze(0)
            x = self.relu(grouped + self.mlps_pos[k](rel_xyz))
            if self.pool_method == 'max_pool':
                x = x.max(dim=3).values                                            # (1, C, M)
            elif self.pool_method == 'avg_pool':
                x = x.mean(dim=3)
            else:
                raise NotImplementedError
            per_scale.append(self.mlps_out[k](x).squeeze(0).permute(1, 0))         # (M, C)
        return torch.cat(per_scale, dim=1)
