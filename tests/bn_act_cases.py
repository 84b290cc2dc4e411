"""Seeded inputs of the op-level tests of csrc/bn_act.hip, shared by tests/test_bn_act_cpu.py -- which checks, with no
kernel involved, the float64 references and the bounds of torch_refs.py -- and tests/test_bn_act_gpu.py.

Every case names the edge it is there for; the shapes are the smallest that reach it, read off the constants of bn_act.hip:
BN_THREADS = 256, statistics chunk >= 4 096 (65 536 halved while fewer than 2 048 workgroups exist), apply tile 4 096
columns, BN_SMALL_MAX = 16 384, max-pool block 1 024 float4, 64-column transpose tile, merge of partials above 1 024.
All arrays are numpy, fp32 unless said otherwise.  mean / invstd of the apply, max-pool and backward cases are INPUTS of those
entry points: the float64 statistics of the first draw of x rounded to fp32; x is then moved off the ReLU threshold."""
import numpy as np

EPS = float(np.float32(1e-5))   # the entry points take eps as a float
RELU_MARGIN = 1e-3          # |pre-activation| of every element of a ReLU case, >> twice the forward bound (some 1e-6)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def stats_of(x):
    """float64 mean, biased variance per channel of x (B, C, P)."""
    xc = np.asarray(x, np.float64).transpose(1, 0, 2).reshape(x.shape[1], -1)
    return xc.mean(1), xc.var(1)


def off_threshold(x, mean, invstd, gamma, beta, per_sample=False):
    """Move the elements of x (B, C, P) whose pre-activation is within RELU_MARGIN of 0 away from it (in place); mean,
    invstd, gamma, beta stay as they are.  Channels with gamma = 0 have pre = beta, which the cases keep off 0."""
    B, C, P = x.shape
    shp = (B, C, 1) if per_sample else (1, C, 1)
    mu, inv = mean.astype(np.float64).reshape(shp), invstd.astype(np.float64).reshape(shp)
    g = np.ones(C) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(C) if beta is None else beta.astype(np.float64)
    sc = inv * g.reshape(1, C, 1)
    for _ in range(8):
        pre = (x.astype(np.float64) - mu) * sc + b.reshape(1, C, 1)
        near = (np.abs(pre) < RELU_MARGIN) & (sc != 0)
        if not near.any():
            return x
        step = np.broadcast_to(4.0 * RELU_MARGIN / np.where(sc != 0, np.abs(sc), 1.0), x.shape)
        x[near] += step[near].astype(np.float32)
    raise AssertionError("could not move x off the ReLU threshold")


# ------------------------------------------------------------------------------------------------ statistics
STATS_CASES = {
    # id: (B, C, P, mean, std, what)
    "second_chunk_of_4": (1, 3, 4100, 0.7, 2.0, "P % 4 == 0, second chunk holds 4 elements: its pivot comes from 4 lanes"),
    "scalar_last_chunk_of_1": (1, 2, 4097, 0.7, 2.0, "P % 4 != 0, the last chunk is one element"),
    "odd_p_chunk_crosses_samples": (3, 2, 1367, 0.7, 2.0, "odd P, chunk 0 spans samples 0..2"),
    "vec_chunk_starts_inside_sample": (5, 3, 1000, 0.7, 2.0, "P % 4 == 0, chunk 1 starts at element 96 of sample 4"),
    "n1": (1, 1, 1, 0.7, 2.0, "n = 1: var = 0 and no unbiased correction"),
    "cancellation_mean1e4": (2, 3, 4100, 1e4, 1.0, "|mean| = 1e4 std: the pivot keeps the variance digits"),
    "outlier_in_pivot": (1, 2, 4096, 0.0, 1.0, "one chunk, 1e6 among its first 256 elements"),
    "chunk_32768": (2, 1024, 16388, 0.7, 2.0, "the intermediate 32 768 chunk (2 x 1 024 workgroups), 134 MB"),
}
MOMENTA = (0.1, 1.0)


def stats_case(name):
    B, C, P, mean, std, _ = STATS_CASES[name]
    rng = np.random.default_rng(_seed(name))
    x = (mean + std * rng.standard_normal((B, C, P), dtype=np.float32)).astype(np.float32)
    if name == "outlier_in_pivot":
        x[0, :, 100] = 1e6
    return dict(B=B, C=C, P=P, x=x, running_mean=rng.standard_normal(C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C).astype(np.float32), nbt=7)


# grouped: G = 3 samples whose means / variances are far apart: any other order of the three momentum updates moves
# running_mean by about momentum * (1 - momentum) * 10
GROUPED_CASES = {"g3_p4100": (3, 2, 4100), "g3_p1367": (3, 3, 1367), "g3_small_p1028": (3, 2, 1028)}
GROUP_MEANS, GROUP_STDS = (0.0, 10.0, -20.0), (1.0, 3.0, 0.5)


def grouped_case(name):
    G, C, P = GROUPED_CASES[name]
    rng = np.random.default_rng(_seed(name))
    x = rng.standard_normal((G, C, P), dtype=np.float32)
    for g in range(G):
        x[g] = GROUP_MEANS[g] + GROUP_STDS[g] * x[g]
    return dict(B=G, C=C, P=P, x=x, running_mean=rng.standard_normal(C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C).astype(np.float32), nbt=7)


# ------------------------------------------------------------------------------------------------ apply
APPLY_P = (3, 4, 4096, 4097, 4100)            # scalar path, one float4, one full tile, scalar past a tile, float4 past a tile
APPLY_AFFINE = ("both", "none", "gamma_only", "beta_only")
APPLY_B, APPLY_C, APPLY_PAD = 2, 4, 8         # y_bstride = C * P + 8


def affine(C, which, rng):
    """gamma with a negative entry and, where a beta keeps the pre-activation off 0, a zero entry (C >= 3); beta off 0."""
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    if C >= 2:
        gamma[1] = -gamma[1]
    if C >= 3 and which == "both":
        gamma[2] = 0.0
    beta = (rng.uniform(0.2, 0.6, C) * np.where(np.arange(C) % 2, -1, 1)).astype(np.float32)
    return (gamma if which in ("both", "gamma_only") else None), (beta if which in ("both", "beta_only") else None)


def apply_case(P, which, per_sample, mean=0.7, relu=True):
    """x (2, 4, P); mean / invstd (C,) or (B, C) with per-sample statistics.  relu=False keeps the near-zero values."""
    rng = np.random.default_rng(P * 10 + APPLY_AFFINE.index(which) * 2 + per_sample + (999 if mean != 0.7 else 0))
    B, C = APPLY_B, APPLY_C
    x = (mean + 2.0 * rng.standard_normal((B, C, P), dtype=np.float32)).astype(np.float32)
    xs = x.reshape(1, B * C, P) if per_sample else x
    m, v = stats_of(xs)
    mean32, invstd32 = m.astype(np.float32), ((v + EPS) ** -0.5).astype(np.float32)
    gamma, beta = affine(C, which, rng)
    if relu:
        off_threshold(x, mean32, invstd32, gamma, beta, per_sample)
    else:
        x[:, :, 0] = mean32.reshape(B, C) if per_sample else mean32[None, :]      # pre-activation exactly beta (or 0)
    return dict(B=B, C=C, P=P, x=x, mean=mean32, invstd=invstd32, gamma=gamma, beta=beta)


# ------------------------------------------------------------------------------------------------ small fused
SMALL_CASES = {
    # id: (B, C, P, per_sample)      n = B * P (or P per sample)
    "n4": (1, 3, 4, 0), "n1028": (1, 3, 1028, 0), "n16384_two_samples": (2, 3, 8192, 0),
    "per_sample_p1028": (3, 2, 1028, 1), "per_sample_p16384": (3, 1, 16384, 1), "per_sample_p4": (3, 3, 4, 1),
}
# the one-launch kernel sums x without a pivot (its own worst case is gamma_u(28) mean|x|) and is held to the bounds of the
# pivoted statistics all the same: its cases keep |mean| <= 4 std
SMALL_GROUP_STDS = (1.0, 3.0, 5.0)
SMALL_REJECTED = {"n16388": (1, 2, 16388, 0), "p_not_multiple_of_4": (1, 2, 1026, 0), "per_sample_p16388": (2, 1, 16388, 1)}


def small_case(name, relu=True):
    B, C, P, per_sample = SMALL_CASES[name]
    rng = np.random.default_rng(_seed(name))
    x = (0.7 + 2.0 * rng.standard_normal((B, C, P), dtype=np.float32)).astype(np.float32)
    if per_sample:
        for g in range(B):
            x[g] = GROUP_MEANS[g] + SMALL_GROUP_STDS[g] * (x[g] - 0.7) / 2.0
    gamma, beta = affine(C, "both", rng)
    if relu:    # the statistics are the kernel's own: move x, recompute, until every element is off the threshold
        for _ in range(8):
            m, v = stats_of(x.reshape(1, B * C, P) if per_sample else x)
            before = x.copy()
            off_threshold(x, m.astype(np.float32), ((v + EPS) ** -0.5).astype(np.float32), gamma, beta, per_sample)
            if np.array_equal(before, x):
                break
    return dict(B=B, C=C, P=P, per_sample=per_sample, x=x, gamma=gamma, beta=beta,
                running_mean=rng.standard_normal(C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C).astype(np.float32), nbt=7)


# ------------------------------------------------------------------------------------------------ max-pool forward
MAX_NS = (1, 2, 3, 4, 5, 8, 16, 32, 64, 128, 255)
MAX_C = 4        # gamma > 0; gamma < 0 (arg-max of y = arg-min of x); gamma = 0 (all tie: arg 0); beta = -10: all negative under ReLU
MAX_GAMMA = np.array([1.3, -0.7, 0.0, 0.9], np.float32)
MAX_BETA = np.array([0.2, -0.1, 0.5, -10.0], np.float32)
MAX_CASES = dict([("m1_ns%d" % ns, (2, 1, ns)) for ns in MAX_NS]
                 + [("ns4_m1025", (1, 1025, 4)), ("ns64_m65", (1, 65, 64)), ("ns5_m257", (1, 257, 5)), ("ns16_m300", (2, 300, 16))])


def tie_pairs(ns):
    """Pairs of slots (s1 < s2) that hold the same maximum: inside one float4, and one pair per butterfly stage of the vector
    kernels (lanes hold 4 slots: xor 1 / 2 / 4 / 8 of the lane = slots 4 / 8 / 16 / 32 apart), started from both sides,
    the pair across the two halves of a 16-lane row (lanes 7, 8), first against last, and one triple."""
    pairs = []
    for d in (1, 2, 4, 8, 16, 32, 64, 128):
        if d < ns:
            for s in (0, ns - 1 - d, (ns // 2) | 1):
                if 0 <= s < ns and (s ^ d) < ns:
                    pairs.append(tuple(sorted((s, s ^ d))))
    if ns >= 2:
        pairs += [(ns // 2 - 1, ns // 2), (0, ns - 1)]
    if ns >= 3:
        pairs.append((ns - 3, ns - 2, ns - 1))
    return sorted(set(pairs))


def _max_x(B, M, ns, seed):
    rng = np.random.default_rng(seed)
    x = (0.7 + 2.0 * rng.standard_normal((B, MAX_C, M, ns), dtype=np.float32)).astype(np.float32)
    m, v = stats_of(x.reshape(B, MAX_C, M * ns))
    mean32, invstd32 = m.astype(np.float32), ((v + EPS) ** -0.5).astype(np.float32)
    return x, mean32, invstd32


def max_case(name):
    B, M, ns = MAX_CASES[name]
    x, mean32, invstd32 = _max_x(B, M, ns, _seed(name))
    off_threshold(x.reshape(B, MAX_C, M * ns), mean32, invstd32, MAX_GAMMA, MAX_BETA)
    return dict(B=B, C=MAX_C, M=M, ns=ns, x=x, mean=mean32, invstd=invstd32, gamma=MAX_GAMMA, beta=MAX_BETA, ties=None)


TIE_NS = (2, 3, 4, 5, 8, 16, 32, 64, 128, 255)


def tie_case(ns):
    """Group m holds tie_pairs(ns)[m]: the extreme x of the group (+1 for gamma >= 0, -1 below for gamma < 0) copied into
    the slots, so that the fp32 activations are identical and beat every other slot by far more than the bound."""
    pairs = tie_pairs(ns)
    B, M = 2, len(pairs)
    x, mean32, invstd32 = _max_x(B, M, ns, 7000 + ns)
    for m, slots in enumerate(pairs):
        for c in range(MAX_C):
            up = MAX_GAMMA[c] >= 0
            ext = x[:, c, m].max(1) + 1.0 if up else x[:, c, m].min(1) - 1.0
            for s in slots:
                x[:, c, m, s] = ext
    off_threshold(x.reshape(B, MAX_C, M * ns), mean32, invstd32, MAX_GAMMA, MAX_BETA)
    for m, slots in enumerate(pairs):          # the nudge is per element: restore exact equality
        for s in slots[1:]:
            x[:, :, m, s] = x[:, :, m, slots[0]]
    return dict(B=B, C=MAX_C, M=M, ns=ns, x=x, mean=mean32, invstd=invstd32, gamma=MAX_GAMMA, beta=MAX_BETA,
                ties=np.array([s[0] for s in pairs]))


# ------------------------------------------------------------------------------------------------ backward
BWD_CASES = {k: v[:3] for k, v in STATS_CASES.items() if k not in ("chunk_32768", "outlier_in_pivot")}
BWD_CASES["p4096_b2"] = (2, 3, 4096)
ROWMAJOR_CASES = [(P, C) for P in (63, 64, 65) for C in (1, 64)]


def bwd_case(B, C, P, relu, which="both", seed=0):
    rng = np.random.default_rng(B * 1000003 + C * 1009 + P + seed)
    x = (0.7 + 2.0 * rng.standard_normal((B, C, P), dtype=np.float32)).astype(np.float32)
    m, v = stats_of(x)
    mean32, invstd32 = m.astype(np.float32), ((v + EPS) ** -0.5).astype(np.float32)
    gamma, beta = affine(C, which, rng)
    if relu:
        off_threshold(x, mean32, invstd32, gamma, beta)
    dy = (rng.standard_normal((B, C, P)) * 10.0 ** rng.uniform(-2, 2, (B, C, P))).astype(np.float32)
    return dict(B=B, C=C, P=P, x=x, dy=dy, mean=mean32, invstd=invstd32, gamma=gamma, beta=beta)


MAXBWD_NS = (3, 4, 5, 64, 255)
MAXBWD_B, MAXBWD_M, MAXBWD_CTOTAL, MAXBWD_C0 = 2, 37, 9, 3      # dpool = channels 3..6 of a (B, 9, M) tensor / of (M, 9) rows
DPOOL_LAYOUTS = ("contiguous", "channel_slice", "transposed_rows")


def maxbwd_case(ns, M=MAXBWD_M):
    B = MAXBWD_B
    x, mean32, invstd32 = _max_x(B, M, ns, 9000 + ns + M)
    off_threshold(x.reshape(B, MAX_C, M * ns), mean32, invstd32, MAX_GAMMA, MAX_BETA)
    rng = np.random.default_rng(9100 + ns)
    wide = (rng.standard_normal((B, MAXBWD_CTOTAL, M)) * 10.0 ** rng.uniform(-2, 2, (B, MAXBWD_CTOTAL, M))).astype(np.float32)
    return dict(B=B, C=MAX_C, M=M, ns=ns, x=x, mean=mean32, invstd=invstd32, gamma=MAX_GAMMA, beta=MAX_BETA, dpool_wide=wide,
                dpool=np.ascontiguousarray(wide[:, MAXBWD_C0:MAXBWD_C0 + MAX_C]))


# ------------------------------------------------------------------------------------------------ statistics from partials
PARTIALS_CASES = {
    # id: (nchunk, chunk, elements of the last chunk, merge route)
    "one_chunk": (1, 128, 128, False), "direct_1024": (1024, 128, 128, False), "merge_1025_short_last": (1025, 128, 40, True),
}
PARTIALS_C = 3


def partials_case(name):
    """Synthetic (mean, M2) partials (C, nchunk, 2): chunk means spread about a channel mean of 100 (so that the spread of
    the chunk means carries variance too)."""
    nchunk, chunk, last, merge = PARTIALS_CASES[name]
    rng = np.random.default_rng(_seed(name))
    cnt = np.full(nchunk, chunk, np.float64)
    cnt[-1] = last
    mean_k = (100.0 + rng.standard_normal((PARTIALS_C, nchunk))).astype(np.float32)
    m2_k = (cnt * rng.uniform(0.5, 2.0, (PARTIALS_C, nchunk))).astype(np.float32)
    return dict(nchunk=nchunk, chunk=chunk, n=int(cnt.sum()), cnt=cnt, merge=merge,
                partial=np.ascontiguousarray(np.stack([mean_k, m2_k], 2)),
                running_mean=rng.standard_normal(PARTIALS_C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, PARTIALS_C).astype(np.float32), nbt=7)
