"""Eval-mode forward time of the RGB trunk (InceptionI3d to Mixed_4f) on one clip at the frame size of bench.py's config c3:
15 frames of 720 x 1280, fp32 or with bf16 payloads (bf16 convolution weights under bfloat16 autocast, as ForwardStep's bf16
configurations run it).

    python tools/i3d_eval.py [--precision fp32|bf16] [--warmup 5] [--iters 20] [--kernel-times] [--json FILE]

Uses only what the package has offered since the trunk's own convolution kernels exist (InceptionI3d(final_endpoint='Mixed_4f'),
.eval(), torch.no_grad, optional bfloat16 autocast), so the same file runs against an older checkout for an A/B: run it from each
tree alternately.  Every timed forward is bracketed by two HIP events on the current stream; the result line is JSON: median / min
/ max ms over the timed forwards, and how often one forward reached each convolution / BatchNorm entry point of the library (the
1x1x1 units' GEMMs are torch launches, not listed).  --kernel-times: after the timed passes, ten more forwards with the library's
per-kernel HIP-event timers on (_lib.kernel_timers) -> ms per forward and launches per forward of every timer row reached (the
timers serialise the launches: these figures say where the time goes, the medians above say how long a forward takes).
MGAR_I3D_FOLD_BN=0 gives the unfused route on a tree that has the fold."""
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
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--kernel-times", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed forwards")

    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.model.backbone import InceptionI3d, Unit3D
    device = torch.device("cuda")
    torch.manual_seed(0)
    net = InceptionI3d(final_endpoint="Mixed_4f")
    net.build()
    net = net.to(device).eval()
    with torch.no_grad():
        for m in net.modules():                       # running statistics away from (0, 1): an eval-mode BatchNorm that does something
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    autocast = args.precision == "bf16"
    if autocast:
        for m in net.modules():
            if isinstance(m, torch.nn.Conv3d):
                m.weight.data = m.weight.data.to(torch.bfloat16)
    x = torch.randn(1, 3, args.frames, args.height, args.width, device=device)

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return net.extract_features(x)

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
        if name.startswith("mgar_conv3d") or name.startswith("mgar_stem_conv3d") or name.startswith("mgar_bn"):
            calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    L.call = counting
    try:
        forward()
    finally:
        L.call = inner
    torch.cuda.synchronize()
    kernels = None
    if args.kernel_times:
        L.kernel_timers(True)
        try:
            forward()
            torch.cuda.synchronize()
            L.kernel_timers()                          # read and reset: the first instrumented forward is not counted
            for _ in range(10):
                forward()
            torch.cuda.synchronize()
            kernels = {k: {"ms_per_forward": round(v[0] / 10.0, 4), "launches_per_forward": v[1] / 10.0}
                       for k, v in sorted(L.kernel_timers().items())}
        finally:
            L.kernel_timers(False)
    res = {"tool": "i3d_eval", "precision": args.precision, "input": list(x.shape), "out_shape": list(out.shape),
           "out_dtype": str(out.dtype).replace("torch.", ""), "warmup": args.warmup, "iters": args.iters,
           "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
           "fold_bn": getattr(Unit3D, "fold_bn_eval", None), "entry_points_per_forward": calls, "kernel_times": kernels,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
