"""Eval-mode forward time of the non-local block (NLBlockND, mode 'dot') at the sizes MGAR-net reaches, fused route
(nonlocal_ops.NL_EVAL_FUSE on: one launch of csrc/nonlocal_eval.hip) against the torch route (switch off) in the same process:

    lidar     3 840 x 96 x 216   the RoI-grid head at config c3, from the (n, 216, 96) rows; the torch route includes the
                                 permute + reshape copy of LiDAR_Backbone._as_grid
    rgb256    256 x 832 x 25     RoIAlign crops of eight clips
    rgb32     32 x 832 x 25      one clip

    python tools/nl_eval.py [--warmup 5] [--iters 30] [--runs 3] [--json FILE]

Every timed forward is bracketed by two HIP events on the current stream.  The two routes alternate, `runs` times each; the
result line is JSON: per size and route the run medians, their median and min-max range, the min / max over all timed forwards, the largest
difference between the two routes' outputs over the largest magnitude, and for the fused route the algebraic bytes (x once +
z once + parameters once) over the median time."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"lidar": (3840, 96, 12, 216, 3, True), "rgb256": (256, 832, 104, 25, 2, False), "rgb32": (32, 832, 104, 25, 2, False)}


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
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.runs < 3:
        raise SystemExit("at least three alternating runs")

    from multimodal_gar_amd import nonlocal_ops as O
    from multimodal_gar_amd.model.backbone import NLBlockND
    from multimodal_gar_amd.model.gat_model import LiDAR_Backbone
    device = torch.device("cuda")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    res = {"tool": "nl_eval", "warmup": args.warmup, "iters": args.iters, "runs": args.runs, "dtype": args.dtype,
           "device": torch.cuda.get_device_name(0)}
    for name, (n, c, ci, p, dim, rows) in SIZES.items():
        torch.manual_seed(0)
        blk = NLBlockND(c, ci, mode='dot', dimension=dim).to(device).eval()
        with torch.no_grad():
            for t in blk.W_z[1].parameters():              # the BatchNorm starts at gamma = beta = 0: make it do something
                t.normal_(1.0, 0.1)
            blk.W_z[1].running_mean.normal_(0.0, 0.1)
            blk.W_z[1].running_var.uniform_(0.5, 1.5)
        x = torch.randn((n, p, c) if rows else (n, c, 5, 5), device=device).to(dtype)

        def forward(fuse):
            O.NL_EVAL_FUSE = fuse
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                if rows:      # what LiDAR_Backbone.forward does on either route
                    return blk.forward_rows(x) if fuse else blk(LiDAR_Backbone._as_grid(x)).reshape(n, c, p)
                return blk(x)
        on, off = forward(True).float(), forward(False).float()
        entry = {"shape": [n, c, ci, p], "max_diff_over_max": float((on - off).abs().max() / off.abs().max())}
        del on, off
        times = {True: [], False: []}
        for _ in range(args.runs):
            for fuse in (False, True):
                times[fuse].append(timed(lambda: forward(fuse), args.warmup, args.iters))
        for fuse, key in ((True, "fused"), (False, "torch")):
            flat = [t for run in times[fuse] for t in run]
            meds = [statistics.median(r) for r in times[fuse]]
            entry[key] = {"run_medians_ms": [round(m, 4) for m in meds], "median_ms": round(statistics.median(meds), 4),
                          "range_ms": round(max(meds) - min(meds), 4), "min_ms": round(min(flat), 4), "max_ms": round(max(flat), 4)}
        nbytes = 2.0 * x.element_size() * n * c * p + 4.0 * (4.0 * ci * c + 3.0 * ci + 3.0 * c)
        entry["fused"]["algebraic_GB"] = round(nbytes / 1e9, 4)
        entry["fused"]["algebraic_TB_per_s"] = round(nbytes / entry["fused"]["median_ms"] / 1e9, 3)
        # the bar: the fused median beats the torch route's by more than the torch route's own min-max range over its runs
        entry["beats_torch_route"] = entry["fused"]["median_ms"] < entry["torch"]["median_ms"] - entry["torch"]["range_ms"]
        res[name] = entry
        del x, blk
        torch.cuda.empty_cache()
    O.NL_EVAL_FUSE = True
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
