"""Time ONE point-wise-convolution entry point of the library on bf16 payloads at given layer shapes:

    python tools/pointwise_bf16.py --entry new|old --shape B,Cin,Cout,P[,prologue] [--shape ...] [--warmup 5] [--iters 20] [--json FILE]

`new` is mgar_pointwise_mfma_bf16_fwd (csrc/pointwise_bf16.hip, bf16 MFMA), `old` is mgar_pointwise_conv_fwd_bf16
(csrc/pointwise_fwd.hip: widened values on the fp32 MFMA).  One entry per process, so an A/B alternates processes; a failing call
ends the process (no retries).  prologue 1 (default) = BatchNorm + ReLU on the input, 0 = none (the first layer of an MLP).  Every
timed launch is bracketed by two HIP events on the current stream; per shape one JSON line: median / min / max ms and GB/s at the
bf16 byte count 2 (Cin + Cout) B P, and TFLOP/s at 2 Cin Cout B P."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTRIES = {"new": "mgar_pointwise_mfma_bf16_fwd", "old": "mgar_pointwise_conv_fwd_bf16"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", required=True, choices=sorted(ENTRIES))
    ap.add_argument("--shape", action="append", required=True, help="B,Cin,Cout,P[,prologue]")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed launches")
    from multimodal_gar_amd import _lib as L
    bf = torch.bfloat16
    name = ENTRIES[args.entry]
    for spec in args.shape:
        nums = [int(v) for v in spec.split(",")]
        b, cin, cout, p = nums[:4]
        prologue = nums[4] if len(nums) > 4 else 1
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((b, cin, p), device="cuda", generator=g).to(bf)
        w = torch.randn((cout, cin), device="cuda", generator=g) * 0.2
        mean = torch.randn((cin,), device="cuda", generator=g) * 0.1
        invstd = torch.randn((cin,), device="cuda", generator=g).abs() + 0.5
        gamma = torch.randn((cin,), device="cuda", generator=g) * 0.1 + 1
        beta = torch.randn((cin,), device="cuda", generator=g) * 0.1
        y = torch.empty((b, cout, p), device="cuda", dtype=bf)
        vec = (L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta), 1) if prologue else (None, None, None, None, 0)
        st = L.stream_of(x)

        def launch():
            L.call(name, L.pptr(x, bf), b, cin, p, L.fptr(w), cin, 1, cout, *vec, L.pptr(y, bf), st)

        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        med = statistics.median(times)
        nbytes, flops = 2.0 * (cin + cout) * b * p, 2.0 * cin * cout * b * p
        line = json.dumps({"tool": "pointwise_bf16", "entry": args.entry, "symbol": name, "B": b, "Cin": cin, "Cout": cout, "P": p,
                           "prologue": prologue, "warmup": args.warmup, "iters": args.iters, "median_ms": round(med, 4),
                           "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "gbs_bf16": round(nbytes / med / 1e6, 1),
                           "tflops": round(flops / med / 1e9, 2), "device": torch.cuda.get_device_name(0)})
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")
        del x, y


if __name__ == "__main__":
    main()
