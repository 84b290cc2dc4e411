"""Time the 1x1x1 units of the I3D trunk on bf16 payloads, one route per process:

    python tools/conv1x1_bf16.py --entry new|affine|mm [--trunk N,P2b,P3,P4 | --shape N,Cin,Cout,P ...] [--warmup 5] [--iters 20]
                                 [--json FILE]

`new` is one launch of mgar_conv1x1_bf16_fwd (csrc/pointwise_wide_bf16.hip) for all samples, `affine` one launch of
mgar_conv1x1_bf16_fwd_affine (BatchNorm + ReLU in the store), `mm` the per-sample torch.mm loop of Unit3D._conv with
MGAR_I3D_K1_BF16=0 (bf16 weight, out= into the sample's slice).  --trunk N,P2b,P3,P4 runs the 29 units up to Mixed_4f at N clips
with P2b columns for Conv3d_2b_1x1, P3 for Mixed_3b / 3c and P4 for Mixed_4b .. 4f (c2: 4,460800,115200,14400); equal shapes are
timed once and carry their count.  One route per process, so an A/B alternates processes; a failing call ends the process (no
retries).  Every timed pass is bracketed by two HIP events on the current stream; per shape one JSON line: median / min / max ms,
GB/s at the bf16 byte count 2 (Cin + Cout) N P, and TFLOP/s at 2 Cin Cout N P."""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTRIES = {"new": "mgar_conv1x1_bf16_fwd", "affine": "mgar_conv1x1_bf16_fwd_affine", "mm": "torch.mm per sample"}


def trunk_shapes(n, p2b, p3, p4):
    """[(N, Cin, Cout, P, count)] of the 1x1x1 units up to Mixed_4f"""
    from multimodal_gar_amd.model.backbone import _I3D_PLAN
    seen = collections.OrderedDict()
    for name, kind, sp in _I3D_PLAN:
        if name == "MaxPool3d_5a_2x2":
            break
        if kind == "conv" and list(sp["k"]) == [1, 1, 1]:
            seen[(n, sp["cin"], sp["cout"], p2b)] = seen.get((n, sp["cin"], sp["cout"], p2b), 0) + 1
        elif kind == "mixed":
            p = p3 if name.startswith("Mixed_3") else p4
            for cout in (sp["oc"][0], sp["oc"][1], sp["oc"][3], sp["oc"][5]):
                seen[(n, sp["cin"], cout, p)] = seen.get((n, sp["cin"], cout, p), 0) + 1
    return [k + (v,) for k, v in seen.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", required=True, choices=sorted(ENTRIES))
    ap.add_argument("--shape", action="append", default=[], help="N,Cin,Cout,P")
    ap.add_argument("--trunk", default=None, help="N,P2b,P3,P4")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed passes")
    shapes = [tuple(int(v) for v in s.split(",")) + (1,) for s in args.shape]
    if args.trunk:
        shapes += trunk_shapes(*(int(v) for v in args.trunk.split(",")))
    if not shapes:
        raise SystemExit("--shape or --trunk")
    from multimodal_gar_amd import _lib as L
    bf = torch.bfloat16
    for n, cin, cout, p, count in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.relu(torch.randn((n, cin, p), device="cuda", generator=g)).to(bf)
        w = torch.randn((cout, cin), device="cuda", generator=g) * (2.0 / cin) ** 0.5
        w16 = w.to(bf)
        scale = torch.rand((cout,), device="cuda", generator=g) + 0.5
        shift = torch.randn((cout,), device="cuda", generator=g) * 0.1
        y = torch.empty((n, cout, p), device="cuda", dtype=bf)
        st = L.stream_of(x)

        if args.entry == "new":
            def launch():
                L.call(ENTRIES["new"], L.pptr(x, bf), n, cin, p, L.fptr(w), cout, L.pptr(y, bf), cout * p, st)
        elif args.entry == "affine":
            def launch():
                L.call(ENTRIES["affine"], L.pptr(x, bf), n, cin, p, L.fptr(w), cout, L.fptr(scale), L.fptr(shift), 1, L.pptr(y, bf),
                       cout * p, st)
        else:
            def launch():
                for i in range(n):
                    torch.mm(w16, x[i], out=y[i])

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
        nbytes, flops = 2.0 * (cin + cout) * n * p, 2.0 * cin * cout * n * p
        line = json.dumps({"tool": "conv1x1_bf16", "entry": args.entry, "symbol": ENTRIES[args.entry], "N": n, "Cin": cin, "Cout": cout,
                           "P": p, "units": count, "warmup": args.warmup, "iters": args.iters, "median_ms": round(med, 4),
                           "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "gbs_bf16": round(nbytes / med / 1e6, 1),
                           "tflops": round(flops / med / 1e9, 2), "device": torch.cuda.get_device_name(0)})
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")
        del x, y


if __name__ == "__main__":
    main()
