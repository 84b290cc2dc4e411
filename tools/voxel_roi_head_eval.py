"""Eval-mode forward time of the Voxel-RoI head (VoxelRCNNHead: RoI-grid pooling of x_conv2/3/4 + shared FC) behind the sparse trunk,
at the voxel-route tensor sizes of bench.py's config c2: 4 clips x 15 frames of 8 192 points, 16 actors per frame
(60 x 16 x 6^3 = 207 360 grid points).

    python tools/voxel_roi_head_eval.py [--precision fp32|bf16] [--warmup 5] [--iters 20] [--json FILE]

Uses only what the package has offered since the voxel route exists (build_network(lidar_model_cfg(p, "voxel")).eval(),
torch.no_grad, optional bfloat16 autocast), so the same file runs against an older checkout for an A/B: run it from each tree
alternately.  MeanVFE and the trunk run ONCE; their outputs (the three feature levels) are held fixed, and every timed forward is
the head alone on a shallow copy of that dict, bracketed by two HIP events on the current stream.  The result line is JSON:
median / min / max ms over the timed forwards, and how often one forward reached each Voxel-RoI pooling / voxel query / BatchNorm
entry point of the library (torch's own batch norm, ReLU, cat and copies of an unfused eval route are torch launches, not listed).
MGAR_VRP_EVAL_FUSE=0 gives the unfused route on a tree that has the inference route."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--actors", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed forwards")

    from multimodal_gar_amd import _lib as L, workload as W
    from multimodal_gar_amd.pcdet.models import build_network
    device = torch.device("cuda")
    ds = W.SyntheticDataset()
    batch = W.make_batch(35, args.clips, args.frames, args.actors, args.points, 64, 96, device)
    data = W.voxelize_batch(batch["points"], ds)
    data["gt_boxes"] = batch["bboxes3d"][:, :args.actors, :].contiguous()
    del batch
    torch.manual_seed(0)
    net = build_network(W.lidar_model_cfg(args.points, "voxel"), 1, ds).to(device).eval()
    autocast = args.precision == "bf16"
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        trunk = net.backbone_3d(net.vfe(data))          # held fixed: the head reads multi_scale_3d_features / _strides, gt_boxes
    levels = {k: (int(v.features.shape[0]), str(v.features.dtype).replace("torch.", "")) for k, v in trunk["multi_scale_3d_features"].items()}

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return net.roi_head(dict(trunk))

    for _ in range(args.warmup):
        out = forward()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = forward()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    calls, inner = {}, L.call

    def counting(name, *a):
        if name.startswith("mgar_voxel_roi_pool") or name.startswith("mgar_voxel_query") or name.startswith("mgar_bn"):
            calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    L.call = counting
    try:
        forward()
    finally:
        L.call = inner
    torch.cuda.synchronize()
    pooled = out["pooled_features"]
    vpm = sys.modules.get("multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules")
    res = {"tool": "voxel_roi_head_eval", "precision": args.precision, "levels": levels, "pooled_shape": list(pooled.shape),
           "pooled_dtype": str(pooled.dtype).replace("torch.", ""), "pooled_contiguous": bool(pooled.is_contiguous()),
           "pooled_abs_mean": round(float(pooled.float().abs().mean()), 6), "warmup": args.warmup, "iters": args.iters,
           "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
           "eval_fuse": getattr(vpm, "MGAR_VRP_EVAL_FUSE", None), "entry_points_per_forward": calls,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
