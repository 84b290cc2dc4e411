"""Eval-mode forward time of the sparse trunk (VoxelBackBone8x) at the voxel-route tensor sizes of bench.py's config c2:
4 clips x 15 frames of 8 192 points, voxelised as the voxel route does (60 clouds, ~4 x 10^5 voxels).

    python tools/voxel_trunk_eval.py [--precision fp32|bf16] [--warmup 5] [--iters 20] [--json FILE]

Uses only what the package has offered since the sparse trunk exists (VoxelBackBone8x(...).eval(), torch.no_grad, optional
bfloat16 autocast), so the same file runs against an older checkout for an A/B: run it from each tree alternately.  Every timed
forward is bracketed by two HIP events on the current stream (rulebooks are rebuilt by every forward, as in a real inference
step); the result line is JSON: median / min / max ms over the timed forwards, and how often one forward reached each
sparse-convolution / BatchNorm entry point of the library (the torch batch norm and ReLU of an unfused eval block are torch
launches, not listed).  MGAR_SPCONV_FOLD_BN=0 gives the unfused route on a tree that has the fold."""
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
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed forwards")

    from multimodal_gar_amd import _lib as L, workload as W
    from multimodal_gar_amd.pcdet.config import EasyDict
    from multimodal_gar_amd.pcdet.models.backbones_3d import VoxelBackBone8x
    device = torch.device("cuda")
    ds = W.SyntheticDataset()
    batch = W.make_batch(35, args.clips, args.frames, 16, args.points, 64, 96, device)
    vox = W.voxelize_batch(batch["points"], ds)
    counts = torch.clamp_min(vox["voxel_num_points"].view(-1, 1), 1.0)
    data = {"batch_size": args.clips * args.frames, "voxel_coords": vox["voxel_coords"],
            "voxel_features": (vox["voxels"].sum(1) / counts).contiguous()}
    del batch, vox
    torch.manual_seed(0)
    net = VoxelBackBone8x(EasyDict(NAME="VoxelBackBone8x"), 4, [int(v) for v in ds.grid_size]).to(device).eval()
    autocast = args.precision == "bf16"

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return net(dict(data))["encoded_spconv_tensor"].features

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
        if name.startswith("mgar_spconv_gather") or name.startswith("mgar_spconv_bf16_fwd") or name.startswith("mgar_bn"):
            calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    L.call = counting
    try:
        forward()
    finally:
        L.call = inner
    torch.cuda.synchronize()
    res = {"tool": "voxel_trunk_eval", "precision": args.precision, "voxels": int(data["voxel_coords"].shape[0]),
           "out_rows": int(out.shape[0]), "out_dtype": str(out.dtype).replace("torch.", ""), "warmup": args.warmup, "iters": args.iters,
           "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
           "fold_bn": getattr(__import__("multimodal_gar_amd.sparse_ops", fromlist=["x"]), "SPCONV_FOLD_BN", None),
           "entry_points_per_forward": calls, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
