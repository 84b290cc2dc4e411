"""Cases, float64 reference, bound and fp32 numpy restatement of the op-level tests of the inference shared-MLP tail
(mgar_pointwise_conv_maxpool_eval_fwd / mgar_pointwise_conv_maxpool_eval_bf16_fwd, csrc/pointwise_fwd.hip MAXPOOL epilogue),
shared by tests/test_mlp_eval_cpu.py (no kernel: the bound is satisfiable, wrong restatements leave it, the cases exercise what
they claim) and tests/test_mlp_eval_gpu.py.

Contract under test, per sample b, output channel o, group m (include/mgar_ops.h), x (B, Cin, M, ns):
    a = relu?((x - mu) sc + sh),  sc = invstd gamma,  sh = beta          (or a = x: the identity prologue)
    z = sum_i W[o, i] a_i;   v = relu?(fmaf(z, scale_o, shift_o));   out = max_s v          (bf16: x bf16, out rounded once)
Reference: the same chain in float64 on the fp32 operands (the bf16-rounded x for bf16).

Bound per element, u = 2^-24, gamma(n) = torch_refs.gamma_u(n):
    E_a   = gamma(4) (|(x - mu) sc| + |sh|)          subtraction, the rounding of sc, product, sum; 0 for the identity
    E_z   = sum_i |W| E_a + gamma(Cin + 2) sum_i |W| (|a| + E_a)     the MFMA chain: one rounding per product, at most Cin per
                                                                      partial sum, one spare for the order inside an MFMA step
    E_v   = |scale| E_z + gamma(1) (|z scale| + |shift| + |scale| E_z)                  one fma; ReLU is 1-Lipschitz
    E_out = max_s E_v                                 max is 1-Lipschitz: no near-tie mask is needed for VALUES
    bf16:   E_out + 2^-8 (|ref| + E_out)              the one output rounding, as voxel_roi_pool_eval_cases.py"""
import functools

import numpy as np

U = 2.0 ** -24
BF16_EPS = 2.0 ** -8
SENTINEL = -77.0
PAD_OUT = 3                      # the pooled buffer of the device tests is (B * Cout * M + PAD_OUT) elements, sentinel-filled

NSAMPLES = (4, 8, 16, 32, 64, 128)

# (B, Cin, Cout, M, ns), prologue in {"bn", "noaffine", "id"}, in_relu, out_relu
# every group width: Cin, Cout <= 16, B = 2, P = M ns no multiple of 128 (ns = 128 cannot help it), the switches rotated
WIDTH_CASES = [((2, 6, 16, 5, 4), "bn", 1, 1), ((2, 9, 13, 9, 8), "id", 0, 1), ((2, 16, 16, 5, 16), "noaffine", 1, 0),
               ((2, 5, 16, 9, 32), "bn", 0, 1), ((2, 12, 16, 7, 64), "bn", 1, 1), ((2, 7, 16, 13, 128), "bn", 1, 0),
               ((2, 3, 11, 3, 128), "id", 0, 0)]
# channel edges: OB = 1 / 2, slab padding (16-channel slabs for OB = 1, 8 for OB = 2), the o < Cout guard
_NS_ROT = (8, 16, 32, 4, 64)
_PRO_ROT = ("bn", "id", "noaffine")
EDGE_CASES = [((1 + (i + j) % 2, cin, cout, 5, _NS_ROT[(i + 2 * j) % 5]), _PRO_ROT[(i + j) % 3], (i + j) % 2, (i + j // 2) % 2)
              for i, cout in enumerate((1, 7, 32, 33, 64)) for j, cin in enumerate((1, 3, 16, 17, 64))]
# more than 8 192 tiles of 128 columns: every wave of the largest grid (2 048 workgroups x 4) takes a second tile, so a wave
# that did not zero its accumulators after the epilogue shows
STRIDE_CASE = ((1, 4, 4, 32801, 32), "bn", 1, 1)
assert STRIDE_CASE[0][3] * STRIDE_CASE[0][4] >= 8200 * 128
CASES = WIDTH_CASES + EDGE_CASES + [STRIDE_CASE]
SMALL_CASES = WIDTH_CASES + EDGE_CASES


def case_id(case):
    (b, cin, cout, m, ns), pro, ir, orl = case
    return "B%d_%dto%d_M%d_ns%d_%s_r%d%d" % (b, cin, cout, m, ns, pro, ir, orl)


def to_bf16(a):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _relu(v, on):
    return np.maximum(v, 0.0) if on else v


@functools.lru_cache(maxsize=None)
def make_case(case, bf16=False):
    """The operands of a case, float32 (x bf16-rounded for bf16), read-only.  x: standard normal plus a per-channel offset.
    (mu, invstd, gamma, beta): per channel, gamma of both signs.  W: standard normal / sqrt(Cin).  scale: both signs, magnitudes
    10^U(-1, 1), different per channel.  shift, even channels: minus a cut between two adjacent group maxima of z scale
    (float64), the one that leaves about 30 % -- at least one -- of the channel's groups with every v < 0, so that out_relu
    cuts whole groups to 0; odd channels: plus 0.2 .. 0.4 of the channel's standard deviation, so the shift takes both signs."""
    (b, cin, cout, m, ns), pro, in_relu, out_relu = case
    rng = np.random.default_rng([7, b, cin, cout, m, ns, in_relu, out_relu])
    x = (rng.standard_normal((b, cin, m, ns)) + rng.uniform(-1, 1, (1, cin, 1, 1))).astype(np.float32)
    if bf16:
        x = to_bf16(x)
    d = {"x": x, "in_relu": in_relu, "out_relu": out_relu, "mean": None, "invstd": None, "gamma": None, "beta": None}
    if pro != "id":
        d["mean"] = rng.uniform(-1, 1, cin).astype(np.float32)
        d["invstd"] = (1.0 / rng.uniform(0.5, 2.0, cin)).astype(np.float32)
        if pro == "bn":
            d["gamma"] = (rng.choice([-1.0, 1.0], cin) * rng.uniform(0.5, 1.5, cin)).astype(np.float32)
            d["beta"] = rng.uniform(-0.5, 0.5, cin).astype(np.float32)
    d["w"] = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    d["scale"] = (rng.choice([-1.0, 1.0], cout) * 10.0 ** rng.uniform(-1, 1, cout)).astype(np.float32)
    if cout > 1:
        d["scale"][:2] = np.abs(d["scale"][:2]) * np.array([1.0, -1.0], np.float32)      # both signs whatever the draw
    a, _ = _prologue(d)
    z = np.einsum("oi,bims->boms", d["w"].astype(np.float64), a)
    zs = z * d["scale"].astype(np.float64)[None, :, None, None]
    gmax = np.sort(zs.max(axis=3).transpose(1, 0, 2).reshape(cout, -1), axis=1)                       # (Cout, B * M) ascending
    k = min(max(1, int(round(0.3 * gmax.shape[1]))), gmax.shape[1] - 1)
    spread = zs.std(axis=(0, 2, 3)) * rng.uniform(0.2, 0.4, cout)
    shift = -0.5 * (gmax[:, k - 1] + gmax[:, k])
    shift = np.where(gmax[:, k - 1] == gmax[:, k], -(gmax[:, k] + spread), shift)   # a tie (Cin = 1 behind a ReLU): cut it too
    shift[1::2] = spread[1::2]                    # odd channels: a positive shift of the size of the channel's spread
    d["shift"] = shift.astype(np.float32)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _prologue(d):
    """-> (a, E_a) float64 (B, Cin, M, ns)"""
    import torch_refs as R
    x = d["x"].astype(np.float64)
    if d["mean"] is None:
        return x, np.zeros_like(x)
    cin = x.shape[1]
    sc = d["invstd"].astype(np.float64) * (d["gamma"].astype(np.float64) if d["gamma"] is not None else 1.0)
    sh = d["beta"].astype(np.float64) if d["beta"] is not None else np.zeros(cin)
    t = (x - d["mean"].astype(np.float64)[None, :, None, None]) * sc[None, :, None, None]
    e = R.gamma_u(4) * (np.abs(t) + np.abs(sh)[None, :, None, None])
    return _relu(t + sh[None, :, None, None], d["in_relu"]), e


@functools.lru_cache(maxsize=None)
def reference(case, bf16=False):
    """-> (ref (B, Cout, M) float64, bound (B, Cout, M) float64, v (B, Cout, M, ns) float64, E_v (B, Cout, M, ns) float64);
    computed once per case and payload and shared: read-only"""
    import torch_refs as R
    d = make_case(case, bf16)
    cin = d["x"].shape[1]
    a, e_a = _prologue(d)
    w64, aw = d["w"].astype(np.float64), np.abs(d["w"].astype(np.float64))
    s64, h64 = d["scale"].astype(np.float64)[None, :, None, None], d["shift"].astype(np.float64)[None, :, None, None]
    z = np.einsum("oi,bims->boms", w64, a)
    e_z = np.einsum("oi,bims->boms", aw, e_a) + R.gamma_u(cin + 2) * np.einsum("oi,bims->boms", aw, np.abs(a) + e_a)
    v = _relu(z * s64 + h64, d["out_relu"])
    e_v = np.abs(s64) * e_z + R.gamma_u(1) * (np.abs(z * s64) + np.abs(h64) + np.abs(s64) * e_z)
    ref, e_out = v.max(axis=3), e_v.max(axis=3)
    if bf16:
        e_out = e_out + BF16_EPS * (np.abs(ref) + e_out)
    for t in (ref, e_out, v, e_v):
        t.setflags(write=False)
    return ref, e_out, v, e_v


def argmax_coverage(cases, ns):
    """Over `cases` with this ns: slots s of the group at which the reference's arg-max falls with a margin to the runner-up
    above twice the larger of the two bounds (so that dropping that slot moves the result out of the bound) -> set of s"""
    seen = set()
    for case in cases:
        if case[0][4] != ns:
            continue
        _, _, v, e_v = reference(case, False)
        order = np.argsort(v, axis=3)
        top, second = order[..., -1], order[..., -2]
        vt = np.take_along_axis(v, top[..., None], 3)[..., 0]
        vs = np.take_along_axis(v, second[..., None], 3)[..., 0]
        clear = (vt - vs) > 2.0 * e_v.max(axis=3)
        seen.update(np.unique(top[clear]).tolist())
    return seen


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _relu32(v):
    return np.where(v > 0, v, np.where(np.isnan(v), v, np.float32(0.0))).astype(np.float32)


def emulate(case, bf16=False, mutant=None):
    """The chain in fp32 numpy as a correct kernel evaluates it: (x - mu) sc + sh with every operation rounded to float32, the
    NaN-passing ReLUs, the sum over i in ascending order with each step an fma (through float64: a product of two float32 is
    exact there), one fmaf for the affine, the max, one rounding to bf16 at the end.  -> (B, Cout, M) float32.
    mutant: one of the wrong restatements of test_mlp_eval_cpu.py --
      "scale_xor1"   scale taken at o ^ 1;            "relu_first"  the output ReLU before the affine;
      "half_group"   max over the first half of the group;          "no_shift"  the shift dropped;
      "bf16_early"   (bf16) the conv output rounded to bf16 before the affine and the max, the pooled value again after --
                     what the unfused route does.  Rounding v itself before the max cannot be told from rounding after it:
                     rounding to nearest is monotone, so it commutes with the max."""
    d = make_case(case, bf16)
    x = d["x"]
    b, cin, m, ns = x.shape
    cout = d["w"].shape[0]
    if d["mean"] is None:
        a = x
    else:
        sc = (d["invstd"] * d["gamma"]).astype(np.float32) if d["gamma"] is not None else d["invstd"]
        sh = d["beta"] if d["beta"] is not None else np.zeros(cin, np.float32)
        a = ((x - d["mean"][None, :, None, None]).astype(np.float32) * sc[None, :, None, None]).astype(np.float32)
        a = (a + sh[None, :, None, None]).astype(np.float32)
        if d["in_relu"]:
            a = _relu32(a)
    z = np.zeros((b, cout, m, ns), np.float32)
    for i in range(cin):
        z = _f32(z.astype(np.float64) + d["w"][None, :, i, None, None].astype(np.float64) * a[:, None, i].astype(np.float64))
    scale, shift = d["scale"], d["shift"]
    if mutant == "scale_xor1":
        scale = scale[np.minimum(np.arange(cout) ^ 1, cout - 1)]
    if mutant == "no_shift":
        shift = np.zeros_like(shift)
    if mutant == "relu_first" and d["out_relu"]:
        z = _relu32(z)
    if mutant == "bf16_early":
        z = to_bf16(z)
    v = _f32(z.astype(np.float64) * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None])
    if d["out_relu"] and mutant != "relu_first":
        v = _relu32(v)
    if mutant == "half_group":
        v = v[..., :ns // 2]
    out = v.max(axis=3)
    return to_bf16(out) if bf16 else out


def used(got, case, bf16=False):
    """max over elements of |got - ref| / bound"""
    ref, lim, _, _ = reference(case, bf16)
    return float((np.abs(np.asarray(got, np.float64) - ref) / lim).max())
