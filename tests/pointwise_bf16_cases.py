"""Cases, operands, float64 reference and per-element bound shared by tests/test_pointwise_bf16_cpu.py and
tests/test_pointwise_bf16_gpu.py for mgar_pointwise_mfma_bf16_fwd (csrc/pointwise_bf16.hip).

The kernel's contract (include/mgar_ops.h):
    a[b,i,p] = bf16(act_i(float(x[b,i,p])))   act_i(v) = relu?(((v - mean_i) * sc_i) + beta_i), sc_i = invstd_i * gamma_i, every
                                              operation rounded to fp32 on its own; identity prologue: a = x
    w~[o,i]  = bf16(w[o * rs + i * cs])
    y[b,o,p] = bf16(sum_i w~[o,i] * a[b,i,p]) fp32 accumulation of exact products, one rounding on store
The rounded operands are restated here in torch (fp32 elementwise operations in the kernel's order, then .bfloat16()); `ref` is
their float64 product.  Bound per element, with S = sum_i |w~| |a|, gamma(k) = k 2^-24 / (1 - k 2^-24), B = gamma(2 (Cin + 2)) S:
    |y - ref| <= B + 2^-8 (|ref| + B)
-- any fp32 accumulation order (the MFMA's internal order included) plus the one store rounding (unit roundoff of bf16: 2^-8);
the bound of DESIGN.md section 3.13d1.  Everything here runs on the CPU and is computed once per (case, variant)."""
import functools

import torch

BF = torch.bfloat16

# (B, Cin, Cout, P, W read transposed)
CASES = (
    (1, 1, 1, 4, False),
    (1, 16, 32, 128, False),
    (3, 35, 20, 4096, False),
    (2, 17, 33, 132, False),
    (1, 64, 64, 124, False),
    (2, 256, 64, 260, False),
    (3, 32, 64, 644, False),        # 128-column tiles straddle samples: 644 = 5 * 128 + 4
    (2, 48, 40, 512, True),         # strides swapped: the weight is stored (Cin, Cout)
)
VARIANTS = ("identity", "bn_relu", "bn_noaffine")   # prologue off; prologue + ReLU; prologue, no ReLU, in_gamma / in_beta NULL


def case_id(case):
    b, cin, cout, p, tr = case
    return "%dx%dx%dx%d%s" % (b, cin, cout, p, "_T" if tr else "")


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def operands(case, variant):
    """-> dict of CPU tensors: x (B, Cin, P) bf16, w_store fp32 as stored, (rs, cs), w (Cout, Cin) fp32 logical, mean, invstd,
    gamma | None, beta | None (Cin) fp32, relu.  randn x, W scaled by 0.2, invstd >= 0.5."""
    b, cin, cout, p, tr = case
    seed = 1000 * CASES.index(case) + 10 * VARIANTS.index(variant)
    x = _rnd(b, cin, p, seed=seed + 1).to(BF)
    w = _rnd(cout, cin, seed=seed + 2, scale=0.2).contiguous()
    ops = {"x": x, "w": w, "relu": 0, "mean": None, "invstd": None, "gamma": None, "beta": None}
    if tr:
        ops["w_store"], ops["strides"] = w.t().contiguous(), (1, cout)
    else:
        ops["w_store"], ops["strides"] = w, (cin, 1)
    if variant != "identity":
        ops["mean"] = _rnd(cin, seed=seed + 3, scale=0.1)
        ops["invstd"] = _rnd(cin, seed=seed + 4).abs() + 0.5
    if variant == "bn_relu":
        ops["gamma"] = _rnd(cin, seed=seed + 5) * 0.1 + 1
        ops["beta"] = _rnd(cin, seed=seed + 6) * 0.1
        ops["relu"] = 1
    return ops


def activated(x, mean, invstd, gamma, beta, relu):
    """The kernel's A operand before its rounding, in fp32: x bf16 (B, Cin, P) -> fp32.  Identity prologue: x widened."""
    v = x.float()
    if mean is None:
        return v
    sc = invstd * (gamma if gamma is not None else torch.ones_like(invstd))          # fp32, one rounding
    sh = beta if beta is not None else torch.zeros_like(invstd)
    v = (v - mean[None, :, None]) * sc[None, :, None] + sh[None, :, None]            # three roundings, the kernel's order
    return torch.relu(v) if relu else v                                              # torch.relu propagates a NaN


def rounded_operands(ops):
    """-> (a (B, Cin, P), w~ (Cout, Cin)) as fp32 tensors holding bf16 values."""
    a = activated(ops["x"], ops["mean"], ops["invstd"], ops["gamma"], ops["beta"], ops["relu"]).to(BF).float()
    return a, ops["w"].to(BF).float()


def gamma_k(k):
    u = k * 2.0 ** -24
    return u / (1.0 - u)


def reference(a, wt):
    """float64 product of the rounded operands and the per-element bound -> (ref, bound), both (B, Cout, P) float64."""
    ref = torch.einsum("oi,bip->bop", wt.double(), a.double())
    s = torch.einsum("oi,bip->bop", wt.double().abs(), a.double().abs())
    big = gamma_k(2 * (a.shape[1] + 2)) * s
    return ref, big + 2.0 ** -8 * (ref.abs() + big)


@functools.lru_cache(maxsize=None)
def expected(case, variant):
    """(ref, bound) of a case, computed once and shared (callers must not modify them)."""
    return reference(*rounded_operands(operands(case, variant)))


def share_of_bound(y, ref, bound):
    """Largest |y - ref| / bound over the elements (y: any float tensor of ref's shape); an element whose bound is 0 must be exact."""
    err = (y.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0
