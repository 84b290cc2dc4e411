"""Eval-mode forward time of the PointNet++ shared MLPs at one clip of bench.py's config c3 (15 frames x 16 384 points, 32 actors):
the level-1 set-abstraction module (npoint 4 096, scales [1+3, 16, 16, 32] at nsample 16 and [1+3, 32, 32, 64] at nsample 32; its
centres are picked once, outside the timing) and the RoI-grid pooling of the per-actor lift (StackSAModuleMSG, 3 scales
[128+3, 32, 32] at nsample 16 on the 6^3 lattice of every box, 128-channel point features), each in fp32 and under bfloat16 autocast.

    python tools/sa_eval.py [--warmup 5] [--iters 20] [--json FILE]

Uses only what the package has offered since these modules exist (.eval(), torch.no_grad, optional bfloat16 autocast), so the
same file runs against an older checkout for an A/B: run it from each tree alternately.  Every timed forward is bracketed by two
HIP events on the current stream; the result line is JSON: per module and payload the median / min / max ms over the timed
forwards and how often one forward reached each point-wise-convolution / BatchNorm entry point of the library (library GEMMs are
torch launches, not listed).  MGAR_MLP_EVAL_FUSE=0 gives the unfused route on a tree that has the inference route."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(forward, warmup, iters):
    for _ in range(warmup):
        forward()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        forward()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def census(L, forward):
    calls, inner = {}, L.call

    def counting(name, *a):
        if name.startswith("mgar_pointwise_conv") or name.startswith("mgar_bn"):
            calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    L.call = counting
    try:
        out = forward()
    finally:
        L.call = inner
    torch.cuda.synchronize()
    return calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--actors", type=int, default=32)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed forwards")

    from multimodal_gar_amd import _lib as L, bn_ops, workload as W
    from multimodal_gar_amd.pcdet.models.roi_heads.voxelrcnn_head import global_grid_points_of_roi
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import PointnetSAModuleMSG
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackSAModuleMSG
    device = torch.device("cuda")
    batch = W.make_batch(35, 1, args.frames, args.actors, args.points, 64, 96, device)
    pts = batch["points"]                                                     # (frames, points, 4)
    xyz = pts[..., :3].contiguous()
    feats1 = pts[..., 3:].permute(0, 2, 1).contiguous()                       # (frames, 1, points)
    sa_cfg = W.lidar_model_cfg(args.points).BACKBONE_3D.SA_CONFIG
    torch.manual_seed(0)
    sa = PointnetSAModuleMSG(npoint=sa_cfg.NPOINTS[0], radii=sa_cfg.RADIUS[0], nsamples=sa_cfg.NSAMPLE[0],
                             mlps=[[1] + list(m) for m in sa_cfg.MLPS[0]], use_xyz=True).to(device).eval()
    pool_cfg = W.lidar_model_cfg(args.points).ROI_HEAD.ROI_GRID_POOL
    pool = StackSAModuleMSG(radii=pool_cfg.POOL_RADIUS, nsamples=pool_cfg.NSAMPLE, mlps=[[128] + list(m) for m in pool_cfg.MLPS],
                            use_xyz=True, pool_method=pool_cfg.POOL_METHOD).to(device).eval()
    with torch.no_grad():
        for m in list(sa.modules()) + list(pool.modules()):                   # running statistics that are not the identity
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        centres = sa.pick_centres(xyz)
        grid, _ = global_grid_points_of_roi(batch["bboxes3d"], pool_cfg.GRID_SIZE)
    new_xyz = grid.view(-1, 3).contiguous()
    per_sample = batch["bboxes3d"].shape[1] * pool_cfg.GRID_SIZE ** 3
    new_cnt = torch.full((args.frames,), per_sample, dtype=torch.int32, device=device)
    xyz_stack = xyz.view(-1, 3).contiguous()
    xyz_cnt = torch.full((args.frames,), args.points, dtype=torch.int32, device=device)
    feats128 = torch.randn((args.frames, 128, args.points), device=device)
    del batch

    res = {"tool": "sa_eval", "frames": args.frames, "points": args.points, "queries": int(new_xyz.shape[0]), "warmup": args.warmup,
           "iters": args.iters, "mlp_eval_fuse": getattr(bn_ops, "MLP_EVAL_FUSE", None), "device": torch.cuda.get_device_name(0)}
    for precision in ("fp32", "bf16"):
        autocast = precision == "bf16"
        f1 = feats1.to(torch.bfloat16) if autocast else feats1
        f128 = feats128.to(torch.bfloat16) if autocast else feats128

        def sa_forward():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                return sa(xyz, f1, new_xyz=centres)[1]

        def pool_forward():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                return pool(xyz=xyz_stack, xyz_batch_cnt=xyz_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, features=f128)[1]

        for name, forward in (("sa_level1", sa_forward), ("roi_grid_pool", pool_forward)):
            entry = timed(forward, args.warmup, args.iters)
            calls, out = census(L, forward)
            entry.update(out_shape=list(out.shape), out_dtype=str(out.dtype).replace("torch.", ""), entry_points_per_forward=calls)
            res["%s_%s" % (name, precision)] = entry
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
