"""Time ONE route of the wide shared-MLP layers of the bf16 PointNet++ trunk at given layer shapes:

    python tools/pointwise_wide_bf16.py --route new|old (--config c2|c5 | --shape KIND,B,Cin,Cout,P[,ns] ...) [--warmup 5] [--iters 20]
                                        [--json FILE]

`new` is csrc/pointwise_wide_bf16.hip as the host code reaches it (bn_ops.conv_bf16_wide: mgar_pointwise_wide_bf16_fwd /
mgar_pointwise_wide_maxpool_bf16_fwd, one launch); `old` is today's route for the same step, as the host code runs it with
MGAR_MLP_BF16_WIDE=0: bn_ops.bn_act (mgar_bn_act_fwd_bf16) + nn_utils.conv1x1 (torch.bmm under autocast) [+ bn_ops.bn_act_maxpool].
KIND: `hidden` = [BN -> ReLU -> conv]; `proj` = conv alone (the FP projections, the first conv of an FP module); `tail` = [BN ->
ReLU -> conv -> BN -> ReLU -> max over ns] (eval mode).  Every BatchNorm is in eval mode, so neither route times a statistics pass
(it is the same pass in both).  --config: the wide layers of SA levels 2-4, the FP hidden layers and the FP projections of
workload.lidar_model_cfg at the configuration's frame count and cloud size.  One route per process, so an A/B alternates
processes; a failing call ends the process (no retries).  Every timed pass is bracketed by two HIP events on the current stream;
per shape one JSON line: median / min / max ms and GB/s at the NEW route's bf16 byte count (2 Cin + 2 Cout per column; tail: 2 Cin
per column + 2 Cout per group).  A shape bn_ops.mlp_bf16_wide_plan refuses (fewer than 65 536 columns) is reported as refused."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FRAMES = {"c2": (60, 8192), "c5": (120, 65536)}      # (clips x frames, points per cloud) of bench.py's bf16 configurations


def config_shapes(config):
    """(KIND, B, Cin, Cout, P, ns) of the wide layers at a configuration; SA MLPs after their folded first layer"""
    b, p = FRAMES[config]
    n1, n2, n3, n4 = p // 4, p // 16, p // 64, p // 256
    out = []
    for npoint, mlps in ((n2, ((64, 64, 128, 16), (64, 96, 128, 32))), (n3, ((128, 196, 256, 16), (128, 196, 256, 32))),
                         (n4, ((256, 256, 512, 16), (256, 384, 512, 32)))):
        for c1, c2, c3, ns in mlps:
            if max(c1, c2) > 64:
                out.append(("hidden", b, c1, c2, npoint * ns, 0))
            out.append(("hidden", b, c2, c3, npoint * ns, 0))
            out.append(("tail", b, c2, c3, npoint * ns, ns))
    # FP modules, deepest first: (known channels, known points, skip channels, unknown points, mlp)
    for ck, m, cs, n, mlp in ((1024, n4, 512, n3, (512, 512)), (512, n3, 256, n2, (512, 512)), (512, n2, 96, n1, (256, 256)),
                              (256, n1, 1, p, (128, 128))):
        out.append(("proj", b, ck, mlp[0], m, 0))
        out.append(("proj", b, cs, mlp[0], n, 0))
        out.append(("hidden", b, mlp[0], mlp[1], n, 0))
    return out


def _bn(c, g):
    bn = nn.BatchNorm2d(c).cuda().eval().requires_grad_(False)
    bn.running_mean.copy_(torch.randn((c,), device="cuda", generator=g) * 0.1)
    bn.running_var.copy_(torch.rand((c,), device="cuda", generator=g) + 0.5)
    bn.weight.copy_(torch.randn((c,), device="cuda", generator=g) * 0.1 + 1)
    bn.bias.copy_(torch.randn((c,), device="cuda", generator=g) * 0.1)
    return bn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", required=True, choices=["new", "old"])
    ap.add_argument("--config", default=None, choices=sorted(FRAMES))
    ap.add_argument("--shape", action="append", default=[], help="KIND,B,Cin,Cout,P[,ns]")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.warmup < 5 or args.iters < 20:
        raise SystemExit("at least 5 warm-up and 20 timed passes")
    shapes = config_shapes(args.config) if args.config else []
    for spec in args.shape:
        f = spec.split(",")
        shapes.append((f[0],) + tuple(int(v) for v in f[1:5]) + (int(f[5]) if len(f) > 5 else 0,))
    if not shapes:
        raise SystemExit("--config or --shape")
    from multimodal_gar_amd import bn_ops
    from multimodal_gar_amd.nn_utils import conv1x1
    bn_ops.MLP_BF16_WIDE = args.route == "new"
    # the kernel is timed at every width it takes: the plan's own channel gates (set FROM this table) are lifted
    bn_ops.WIDE_PLAN_MAX_IN, bn_ops.WIDE_PLAN_MAX_OUT = bn_ops.WIDE_MAX_IN, bn_ops.WIDE_MAX_OUT
    bf = torch.bfloat16
    for kind, b, cin, cout, p, ns in shapes:
        if kind not in ("hidden", "proj", "tail") or (kind == "tail") != bool(ns):
            raise SystemExit("bad shape %r" % ((kind, b, cin, cout, p, ns),))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((b, cin, p // ns, ns) if ns else (b, cin, p, 1), device="cuda", generator=g).to(bf)
        conv = nn.Conv2d(cin, cout, 1, bias=False).cuda().requires_grad_(False)
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=g) * 0.2)
        bn = None if kind == "proj" else _bn(cin, g)
        bn2 = _bn(cout, g) if kind == "tail" else None
        relu = nn.ReLU()
        others = () if bn is None else (relu,) + ((relu,) if bn2 is not None else ())

        if args.route == "new":
            def step():
                return bn_ops.conv_bf16_wide(x, conv, bn, bn is not None, bn2, bn2 is not None, pool=bn2 is not None, others=others)
        else:
            def step():
                a = x if bn is None else bn_ops.bn_act(x, bn, True)
                y = conv1x1(conv, a)
                return y if bn2 is None else bn_ops.bn_act_maxpool(y, bn2, True)

        rec = {"tool": "pointwise_wide_bf16", "route": args.route, "config": args.config, "kind": kind, "B": b, "Cin": cin, "Cout": cout,
               "P": p, "ns": ns, "warmup": args.warmup, "iters": args.iters}
        with torch.no_grad(), torch.autocast("cuda", dtype=bf):
            out = step()
            if out is None:
                rec["refused"] = True       # the plan's gates (fewer than 65 536 columns): the model keeps today's route here
            else:
                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                times = []
                for _ in range(args.iters):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    step()
                    t1.record()
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1))
                med = statistics.median(times)
                nbytes = 2.0 * cin * b * p + 2.0 * cout * b * (p // ns if ns else p)
                rec.update(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                           gbs_bf16=round(nbytes / med / 1e6, 1), tflops=round(2.0 * cin * cout * b * p / med / 1e9, 2),
                           device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")
        del x, out


if __name__ == "__main__":
    main()
