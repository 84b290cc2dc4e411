"""Case tables, seeded inputs, float64 references and rounding-count bounds of the op-level tests of csrc/scene_ops.hip
(scene BatchNorm, pair geometry, Gram matrix on packed scene rows), shared by tests/test_scene_ops_cpu.py -- which checks,
with no kernel involved, that every bound is satisfiable (the kernels' arithmetic restated in fp32 numpy stays inside it)
and that it bites (a planted defect exceeds it) -- and tests/test_scene_ops_gpu.py.

Every case names the code path it is there for.  All inputs are fp32 numpy arrays; references are float64 numpy.  The
bounds are DESIGN.md section 5e evaluated in float64: gamma_k = k u / (1 - k u), u = 2^-24, k the number of roundings on
the kernel's summation path, times the sum of the absolute values of the terms."""
import numpy as np
import torch

import fusion_cases as FC
from torch_refs import gamma_u

U32 = 2.0 ** -24


def offsets(counts):
    so = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    do = np.concatenate([[0], np.cumsum(np.square(counts))]).astype(np.int64)
    return so, do[:-1], int(do[-1])


# ------------------------------------------------------------------------------------------------ scene BatchNorm
# grid (S, C / 64), one wave per (scene, 64 channels), lanes along channels; serial sums over the scene's rows.
_RAGGED = [2, 128, 3, 65, 0, 5]     # smallest legal scene, full capacity, more than a wave's worth of rows, empty in the middle
BN_CASES = {
    "ragged_C64": dict(counts=_RAGGED, C=64, kind="normal"),                     # one channel block
    "ragged_C192_cancel": dict(counts=_RAGGED, C=192, kind="cancel"),            # three channel blocks; N(100, 0.01^2)
    "trailing_empty_C64_cancel": dict(counts=[7, 0], C=64, kind="cancel"),       # a trailing empty scene
    "trailing_empty_C192": dict(counts=[7, 0], C=192, kind="normal"),
    "single_scene_C64": dict(counts=[5], C=64, kind="normal"),                   # S = 1
    "single_scene_C192_cancel": dict(counts=[5], C=192, kind="cancel"),
    "one_row_scene_C64": dict(counts=[4, 1, 3], C=64, kind="normal"),            # n_s = 1: y = beta, no running update
}
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def bn_inputs(case, seed=3):
    rng = np.random.default_rng(seed)
    rows, C = sum(case["counts"]), case["C"]
    if case["kind"] == "cancel":
        x = 100.0 + 0.01 * rng.standard_normal((rows, C))
    else:
        x = rng.standard_normal((rows, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.0, 1.0, C)
    f = np.float32
    return dict(x=x.astype(f), gamma=rng.uniform(0.5, 1.5, C).astype(f) * np.where(rng.random(C) < 0.3, -1, 1).astype(f),
                beta=rng.standard_normal(C).astype(f), dy=rng.standard_normal((rows, C)).astype(f),
                running_mean=rng.standard_normal(C).astype(f), running_var=rng.uniform(0.5, 1.5, C).astype(f),
                num_batches_tracked=11)


def bn_ref(counts, inp, eps=BN_EPS, momentum=BN_MOMENTUM, drop_row=False, biased_running=False):
    """float64 reference of mgar_scene_bn_fwd / _bwd with its bounds.  Planted defects: drop_row leaves the last row of
    every scene out of its sums (mean, variance, the two backward sums); biased_running feeds the biased variance to the
    running update."""
    x, dy = inp["x"].astype(np.float64), inp["dy"].astype(np.float64)
    g, b = inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64)
    S, C = len(counts), x.shape[1]
    so, _, _ = offsets(counts)
    out = {k: np.zeros_like(x) for k in ("y", "y_bound", "dx", "dx_bound")}
    for k in ("mean", "var", "invstd", "mean_bound", "var_bound", "invstd_bound"):
        out[k] = np.zeros((S, C))
    rm, rv = inp["running_mean"].astype(np.float64), inp["running_var"].astype(np.float64)
    rm_b, rv_b = np.zeros(C), np.zeros(C)
    dgamma, dbeta, dgamma_b, dbeta_b, dgamma_abs, dbeta_abs = (np.zeros(C) for _ in range(6))
    steps = 0
    m = momentum
    for s, n in enumerate(counts):
        if n == 0:
            continue
        sl = slice(so[s], so[s] + n)
        xs, gs = x[sl], dy[sl]
        if n == 1:
            out["mean"][s] = xs[0]
            out["y"][sl] = b
            dbeta += gs[0]; dbeta_abs += np.abs(gs[0])
            continue
        red = slice(0, n - 1) if drop_row else slice(0, n)
        mean = xs[red].sum(0) / n
        var = ((xs[red] - mean) ** 2).sum(0) / n
        inv = 1.0 / np.sqrt(var + eps)
        # mean: n - 1 adds and a division
        d_mean = gamma_u(n) * np.abs(xs).sum(0) / n
        # var: sum (x - m^)^2 / n = var + (mean - m^)^2 exactly; subtraction, square, n chain steps, division
        d_var = d_mean ** 2 + gamma_u(n + 3) * (var + d_mean ** 2)
        v_lo = np.maximum(var - d_var, 0.0) + eps
        # invstd = 1 / sqrt(var^ + eps): the slope of (v + eps)^-1/2 at the low end, then add, sqrt, divide
        d_inv = 0.5 * d_var * v_lo ** -1.5 + gamma_u(3) * v_lo ** -0.5
        out["mean"][s], out["var"][s], out["invstd"][s] = mean, var, inv
        out["mean_bound"][s], out["var_bound"][s], out["invstd_bound"][s] = d_mean, d_var, d_inv
        cen = xs - mean
        A, Iv = np.abs(cen) + d_mean, inv + d_inv
        out["y"][sl] = cen * inv * g + b
        # y = fma(x - m^, invstd^ gamma, beta): subtraction, coefficient product, fma
        out["y_bound"][sl] = np.abs(g) * (d_mean * Iv + np.abs(cen) * d_inv) + gamma_u(3) * A * Iv * np.abs(g) + U32 * np.abs(b)
        # running statistics: coefficient 1 - m, two products, one add per step; n / (n - 1) and its product for the variance
        unb = var * (1.0 if biased_running else n / (n - 1.0))
        d_unb = (d_var + gamma_u(2) * (var + d_var)) * n / (n - 1.0)
        rm_b = (1 - m) * rm_b + m * d_mean + gamma_u(4) * ((1 - m) * (np.abs(rm) + rm_b) + m * (np.abs(mean) + d_mean))
        rv_b = (1 - m) * rv_b + m * d_unb + gamma_u(4) * ((1 - m) * (np.abs(rv) + rv_b) + m * (unb + d_unb))
        rm = (1 - m) * rm + m * mean
        rv = (1 - m) * rv + m * unb
        steps += 1
        # backward: a = sum dy (n - 1 adds), b = sum dy xhat (n fma steps on xhat = (x - m^) invstd^, two roundings)
        xhat = cen * inv
        d_xhat = d_mean * Iv + np.abs(cen) * d_inv + gamma_u(2) * A * Iv
        a_sum, b_sum = gs[red].sum(0), (gs[red] * xhat[red]).sum(0)
        d_a = gamma_u(n) * np.abs(gs).sum(0)
        d_b = (np.abs(gs) * d_xhat).sum(0) + gamma_u(n) * (np.abs(gs) * (np.abs(xhat) + d_xhat)).sum(0)
        dbeta += a_sum; dgamma += b_sum
        dbeta_b += d_a; dgamma_b += d_b
        dbeta_abs += np.abs(a_sum) + d_a; dgamma_abs += np.abs(b_sum) + d_b
        am, bm = a_sum / n, b_sum / n
        d_am = (d_a + U32 * (np.abs(a_sum) + d_a)) / n
        d_bm = (d_b + U32 * (np.abs(b_sum) + d_b)) / n
        gi = g * inv
        d_gi = np.abs(g) * d_inv + U32 * np.abs(g) * Iv
        inner = gs - am - xhat * bm
        # (dy - am) - xhat bm: two subtractions and a product
        d_inner = (d_am + np.abs(xhat) * d_bm + d_xhat * (np.abs(bm) + d_bm)
                   + gamma_u(3) * (np.abs(gs) + np.abs(am) + d_am + (np.abs(xhat) + d_xhat) * (np.abs(bm) + d_bm)))
        out["dx"][sl] = gi * inner
        out["dx_bound"][sl] = np.abs(gi) * d_inner + d_gi * (np.abs(inner) + d_inner) + U32 * (np.abs(gi) + d_gi) * (np.abs(inner) + d_inner)
    # the per-scene partials are summed over all S scenes in ascending order: S adds at the most
    out.update(running_mean=rm, running_var=rv, running_mean_bound=rm_b, running_var_bound=rv_b, steps=steps,
               dgamma=dgamma, dbeta=dbeta, dgamma_bound=dgamma_b + gamma_u(S) * dgamma_abs,
               dbeta_bound=dbeta_b + gamma_u(S) * dbeta_abs)
    return out


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def bn_fp32(counts, inp, eps=BN_EPS, momentum=BN_MOMENTUM):
    """The kernels' arithmetic of csrc/scene_ops.hip restated in fp32 numpy, operation for operation."""
    f = np.float32
    x, dy, g, b = inp["x"], inp["dy"], inp["gamma"], inp["beta"]
    S, C = len(counts), x.shape[1]
    so, _, _ = offsets(counts)
    y, dx = np.zeros_like(x), np.zeros_like(x)
    mean_s, var_s, inv_s = (np.zeros((S, C), f) for _ in range(3))
    pg, pb = np.zeros((S, C), f), np.zeros((S, C), f)
    rm, rv = inp["running_mean"].copy(), inp["running_var"].copy()
    m, steps = f(momentum), 0
    for s, n in enumerate(counts):
        if n == 0:
            continue
        xs, gs = x[so[s]:so[s] + n], dy[so[s]:so[s] + n]
        if n == 1:
            mean_s[s] = xs[0]; y[so[s]] = b; pb[s] = gs[0]
            continue
        acc = np.zeros(C, f)
        for r in range(n):
            acc = acc + xs[r]
        mean = acc / f(n)
        m2 = np.zeros(C, f)
        for r in range(n):
            d = xs[r] - mean
            m2 = _fma32(d, d, m2)
        var = m2 / f(n)
        inv = f(1) / np.sqrt(var + f(eps))
        a = inv * g
        for r in range(n):
            y[so[s] + r] = _fma32(xs[r] - mean, a, b)
        mean_s[s], var_s[s], inv_s[s] = mean, var, inv
        rm = (f(1) - m) * rm + m * mean
        rv = (f(1) - m) * rv + m * (var * (f(n) / f(n - 1)))
        steps += 1
        sa, sb = np.zeros(C, f), np.zeros(C, f)
        for r in range(n):
            sa = sa + gs[r]
            sb = _fma32(gs[r], (xs[r] - mean) * inv, sb)
        pg[s], pb[s] = sb, sa
        am, bm, gi = sa / f(n), sb / f(n), g * inv
        for r in range(n):
            dx[so[s] + r] = gi * ((gs[r] - am) - ((xs[r] - mean) * inv) * bm)
    dgamma, dbeta = np.zeros(C, f), np.zeros(C, f)
    for s in range(S):
        dgamma = dgamma + pg[s]; dbeta = dbeta + pb[s]
    return dict(y=y, mean=mean_s, var=var_s, invstd=inv_s, running_mean=rm, running_var=rv, steps=steps, dx=dx,
                dgamma=dgamma, dbeta=dbeta)


BN_CHECKED = ("y", "mean", "var", "invstd", "running_mean", "running_var", "dx", "dgamma", "dbeta")


def worst_ratio(got, ref, what):
    """max |got - ref| / bound over the elements of `what` (0 / 0 counts as 0: exact where the bound is 0)."""
    err = np.abs(np.asarray(got, np.float64) - ref[what])
    bound = ref[what + "_bound"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ pair geometry
# One wave per row, lanes striding over j: n = 1, 2, 64, 65 (second trip), 128, an empty scene, 3; 263 rows (263 % 4 = 3).
GEOM_COUNTS = [1, 2, 64, 65, 128, 0, 3]
GEOM_CASES = {
    "duplicates": dict(scale=10.0, duplicates=True),     # equal centres: |ci|^2 + |cj|^2 - 2 ci.cj cancels to ~0, the clamp path
    "magnitude_1e3": dict(scale=1e3, duplicates=False),  # centres of magnitude 1e3: why the distance is evaluated in double
}
# planted in the first rows of every scene of at least 6 boxes: A, A again (identical), nested in A, disjoint from A,
# touching A along x = 50 (zero intersection), one pixel wide -- all of positive area
SPECIAL_BOXES = np.array([[10, 10, 50, 60], [10, 10, 50, 60], [20, 20, 30, 30], [200, 200, 260, 300], [50, 10, 90, 60],
                          [30, 5, 31, 100]], np.float32)


def geom_inputs(case, seed=4):
    rng = np.random.default_rng(seed)
    rows = sum(GEOM_COUNTS)
    so, _, _ = offsets(GEOM_COUNTS)
    centres = (rng.standard_normal((rows, 3)) * case["scale"]).astype(np.float32)
    xy = rng.uniform(0, 300, (rows, 2)); wh = rng.uniform(2, 120, (rows, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    for s, n in enumerate(GEOM_COUNTS):
        if n >= 6:
            boxes[so[s]:so[s] + 6] = SPECIAL_BOXES
        if case["duplicates"] and n >= 2:
            centres[so[s] + n - 1] = centres[so[s]]                    # first and last actor at the same place
            if n >= 64:
                centres[so[s] + 10:so[s] + 20] = centres[so[s] + 5]    # a cluster of eleven
    assert ((boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])).all()
    return centres, boxes


def de_ref(c):
    """float64 restatement for one scene: sqrt(max(0, |ci|^2 + |cj|^2 - 2 ci.cj)), zero diagonal."""
    c = c.astype(np.float64)
    sq = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    dot = c[:, None, 0] * c[None, :, 0] + c[:, None, 1] * c[None, :, 1] + c[:, None, 2] * c[None, :, 2]
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * dot, 0.0))
    np.fill_diagonal(d, 0.0)
    return d


DE_NEAR_ZERO = 1e-3


def de_close(got, ref):
    """within one fp32 ulp of the float64 value; 1e-6 absolute where that value is below DE_NEAR_ZERO (the entries of
    duplicate centres, where the squared distance cancels to ~0 and is clamped)."""
    err = np.abs(got.astype(np.float64) - ref)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return (err <= np.where(ref < DE_NEAR_ZERO, 1e-6, ulp)).all(), float(err.max(initial=0.0))


def giou_fp32_error(b):
    """What torch's own fp32 _giou_batched (model/gat_model.py, on the CPU) differs from float64 by on one scene's boxes:
    the measured figure the device test doubles."""
    from multimodal_gar_amd.model.gat_model import _giou_batched
    got = _giou_batched(torch.from_numpy(np.ascontiguousarray(b, np.float32))[None])[0].double().numpy()
    return float(np.abs(got - giou(b, np.float64)).max())


def giou(b, dtype):
    """_giou_batched of model/gat_model.py for one scene in numpy at `dtype`, the same operation order."""
    b = b.astype(dtype)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(b[:, None, :2], b[None, :, :2]); rb = np.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    union = area[:, None] + area[None, :] - inter
    lti = np.minimum(b[:, None, :2], b[None, :, :2]); rbi = np.maximum(b[:, None, 2:], b[None, :, 2:])
    whi = np.clip(rbi - lti, 0, None)
    areai = whi[..., 0] * whi[..., 1]
    return inter / union - (areai - union) / areai


# ------------------------------------------------------------------------------------------------ Gram matrix
# One wave per row, lanes along j (two column registers), scalar x_i in steps of 16; backward lanes along d in steps of 256.
def _gram_cases():
    lists = []
    for c in FC.DAFM_CASES.values():
        if c["counts"] not in lists:
            lists.append(c["counts"])
    return {"n%s_D%d" % ("_".join(map(str, cnt)), D): dict(counts=cnt, D=D) for cnt in lists for D in (64, 192, 512)}


GRAM_CASES = _gram_cases()


def gram_inputs(case, seed=8):
    rng = np.random.default_rng(seed)
    rows = sum(case["counts"])
    _, _, pairs = offsets(case["counts"])
    return rng.standard_normal((rows, case["D"])).astype(np.float32), rng.standard_normal(pairs).astype(np.float32)  # dG: not symmetric


def gram_ref(counts, x, dg, drop_row=False, no_transpose=False):
    """float64 reference with bounds.  Forward: a chain of D fma steps, gamma_D sum_d |x_id x_jd|.  Backward: one add for
    w_ij = dG_ij + dG_ji, then n fma steps, gamma_(n+1) sum_j |w_ij| |x_jd|.  Planted defects: drop_row leaves the last row j
    out of the backward's sum; no_transpose leaves dG_ji out."""
    so, do, pairs = offsets(counts)
    x64 = x.astype(np.float64)
    D = x.shape[1]
    out = dict(g=np.zeros(pairs), g_bound=np.zeros(pairs), dx=np.zeros_like(x64), dx_bound=np.zeros_like(x64))
    for s, n in enumerate(counts):
        if n == 0:
            continue
        xs = x64[so[s]:so[s] + n]
        out["g"][do[s]:do[s] + n * n] = (xs @ xs.T).reshape(-1)
        out["g_bound"][do[s]:do[s] + n * n] = (gamma_u(D) * (np.abs(xs) @ np.abs(xs).T)).reshape(-1)
        gm = dg[do[s]:do[s] + n * n].astype(np.float64).reshape(n, n)
        w = gm if no_transpose else gm + gm.T
        w_true = gm + gm.T
        out["dx"][so[s]:so[s] + n] = (w[:, :n - 1] @ xs[:n - 1]) if drop_row else w @ xs
        out["dx_bound"][so[s]:so[s] + n] = gamma_u(n + 1) * (np.abs(w_true) @ np.abs(xs))
    return out


def gram_fp32(counts, x, dg):
    """The two kernels restated in fp32 numpy: fma chains over d (forward) and over j (backward), ascending."""
    so, do, pairs = offsets(counts)
    g, dx = np.zeros(pairs, np.float32), np.zeros_like(x)
    for s, n in enumerate(counts):
        if n == 0:
            continue
        xs = x[so[s]:so[s] + n]
        acc = np.zeros((n, n), np.float32)
        for d in range(x.shape[1]):
            acc = _fma32(xs[:, None, d], xs[None, :, d], acc)
        g[do[s]:do[s] + n * n] = acc.reshape(-1)
        gm = dg[do[s]:do[s] + n * n].reshape(n, n)
        w = gm + gm.T
        a = np.zeros((n, x.shape[1]), np.float32)
        for j in range(n):
            a = _fma32(w[:, j:j + 1], xs[j:j + 1], a)
        dx[so[s]:so[s] + n] = a
    return dict(g=g, dx=dx)
