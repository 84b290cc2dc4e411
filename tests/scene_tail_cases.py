"""Cases, seeded inputs, the float64 reference and the rounding-count bounds of the eval-mode fusion-net tail
(csrc/scene_tail_eval.hip, multimodal_gar_amd/scene_tail_ops.py), shared by tests/test_scene_tail_cpu.py and
tests/test_scene_tail_gpu.py.  Plain torch / numpy on the CPU; no kernel is involved here.

The reference is forward_per_scene in eval mode as a float64 chain on the fp32 inputs: Dv = <x_i, x_j> / (|x_i| |x_j|),
a = D_embed([Dv, Dg]) with a_ii = 1, group id = smallest j with a_ij >= 0.5, group max-pool, column maxima and block sum.

Two families.  (a) "sep": rows are a few orthogonal prototypes plus small noise and D_embed is set by hand so that members of
one prototype get a ~ 1 and the others a ~ 0: every off-diagonal entry of the float64 adjacency is farther from 0.5 than the
margin m = 4 x its value bound (asserted for every case on the CPU), so group ids, pooled rows and column maxima must match
exactly.  (b) "rnd": random rows and parameters: values are compared everywhere, ids and pooled rows on the rows whose whole
reference adjacency row keeps the margin, which are at least 90 % of all rows (asserted on the CPU with these seeds).

Value bound, per element, u = 2^-24, g(k) = gamma_u(k) = k u / (1 - k u), for the kernel's arithmetic:
  dot      one fmaf chain of D steps:                       |d dot| <= g(D) sum_d |x_id x_jd|
  |x_i|    chain of D positive terms, sqrt, one rounding:   relative r_n = g(D) / (2 (1 - g(D))) + u
  Dv       dot / (|x_i| |x_j|): product and quotient round once each:
           e_dv = (g(D) sum|x_id x_jd| / (|x_i||x_j|) + |Dv| (2 r_n + 2 u)) (1 + 2^-10)      (2^-10 covers the cross terms)
  hidden 0 z = fma(w_g, Dg, fma(w_v, Dv, b)):               e_z = |w_v| e_dv + g(2) (|w_v| (|Dv| + e_dv) + |w_g Dg| + |b|)
  hidden H pre_k likewise (ReLU is 1-Lipschitz), then a chain of H fmaf onto b2:
           e_z = sum |w2_k| e_k + g(H) (|b2| + sum |w2_k| (|h_k| + e_k))
  sigmoid  s = 1 / (1 + exp(-z)): the slope is at most 1/4; exp within one ulp (2 u relative), the addition and the division
           one rounding each: |d s| <= s (1 - s) 2 u + 2 u s <= 3 u:   e_a = e_z / 4 + 3 u + 2^-149
  diagonal exactly 1.
  card sum n row chains of n additions, then a chain of n:  sum e_a + g(2 n) sum (|a| + e_a)
Dg is an input of the kernel (fp32 GIoU of real boxes) and carries no error of its own."""
import numpy as np
import torch
import torch.nn as nn

import scene_cases as SC
from torch_refs import gamma_u

U32 = 2.0 ** -24
SIZES = (2, 3, 31, 32, 33, 63, 64, 65, 127, 128)
_C1, _C2, _C3 = [2, 3, 31, 32, 33, 63], [64, 65, 127, 128], [128, 2, 65, 3]
_SHAPES = [(_C1, 64, 0, 0), (_C1, 512, 1, 4), (_C2, 64, 5, 4), (_C2, 512, 0, 0), (_C3, 512, 5, 8), (_C3, 64, 1, 0)]
CASES = [dict(family=f, counts=c, D=d, mnp=max(c) + extra, hidden=h, seed=11 + 7 * i + (100 if f == "rnd" else 0))
         for f in ("sep", "rnd") for i, (c, d, extra, h) in enumerate(_SHAPES)]
MIN_MARGIN_ROWS = 0.9


def case_id(case):
    return "%s_n%s_D%d_mnp%d_h%d" % (case["family"], "-".join(map(str, case["counts"])), case["D"], case["mnp"], case["hidden"])


def _boxes(rng, n):
    xy = rng.uniform(0, 300, (n, 2)); wh = rng.uniform(2, 120, (n, 2))
    b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    if n >= 6:
        b[:6] = SC.SPECIAL_BOXES           # identical, nested, disjoint, touching, one pixel wide
    return b


def _params(case, rng):
    """fp32 D_embed parameters: dict(w1 (H, 2), b1 (H), w2 (H), b2 ()) or, hidden == 0, dict(w (2,), b ())."""
    h, f = case["hidden"], np.float32
    if case["family"] == "sep":
        if h == 0:
            return dict(w=np.array([8.0, 0.5], f), b=f(-4.0))
        w1 = np.stack([[8.0, 0.25], [-8.0, 0.25]] + [[0.1, 0.1]] * (h - 2)).astype(f)
        b1 = np.array([-4.0, 4.0] + [0.05 * k for k in range(2, h)], f)
        w2 = np.array([2.0, -2.0] + [0.1] * (h - 2), f)
        return dict(w1=w1, b1=b1, w2=w2, b2=f(0.0))
    sign = lambda: rng.choice([-1.0, 1.0])                                           # noqa: E731
    if h == 0:
        return dict(w=rng.standard_normal(2).astype(f), b=f(sign() * rng.uniform(0.5, 1.5)))
    return dict(w1=rng.standard_normal((h, 2)).astype(f), b1=rng.standard_normal(h).astype(f),
                w2=rng.standard_normal(h).astype(f), b2=f(sign() * rng.uniform(0.5, 1.5)))


def param_block(p):
    """The kernel's parameter block (scene_tail_ops.embed_params) as fp32 numpy."""
    if "w" in p:
        return np.concatenate([p["w"], [p["b"]]]).astype(np.float32)
    return np.concatenate([p["w1"].reshape(-1), p["b1"], p["w2"], [p["b2"]]]).astype(np.float32)


def make_d_embed(p):
    """The nn.Sequential GAR_Fusion_Net3 would hold, with these parameters."""
    with torch.no_grad():
        if "w" in p:
            m = nn.Sequential(nn.Linear(2, 1), nn.Sigmoid())
            m[0].weight.copy_(torch.from_numpy(p["w"]).view(1, 2)); m[0].bias.fill_(float(p["b"]))
        else:
            h = p["w1"].shape[0]
            m = nn.Sequential(nn.Linear(2, h), nn.ReLU(), nn.Linear(h, 1), nn.Sigmoid())
            m[0].weight.copy_(torch.from_numpy(p["w1"])); m[0].bias.copy_(torch.from_numpy(p["b1"]))
            m[2].weight.copy_(torch.from_numpy(p["w2"]).view(1, h)); m[2].bias.fill_(float(p["b2"]))
    return m


_INPUTS = {}


def inputs(case):
    """dict(x (rows, D) fp32, dg (pairs,) fp32 packed, boxes (rows, 4), params): computed once per case and shared."""
    key = case_id(case)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.default_rng(case["seed"])
    D, xs, dgs, bs = case["D"], [], [], []
    for n in case["counts"]:
        if case["family"] == "sep":
            n_proto = min(4, max(1, n // 2))
            width = D // 4
            protos = np.zeros((n_proto, D))
            for p in range(n_proto):                                  # disjoint coordinate blocks: exactly orthogonal
                protos[p, p * width:(p + 1) * width] = rng.standard_normal(width)
            which = rng.integers(0, n_proto, n)
            x = (protos[which] + 0.01 * rng.standard_normal((n, D))) * rng.uniform(0.5, 2.0, (n, 1))
        else:
            x = rng.standard_normal((n, D)) * rng.uniform(0.5, 2.0, (n, 1))
        b = _boxes(rng, n)
        xs.append(x.astype(np.float32)); bs.append(b)
        dgs.append(SC.giou(b, np.float32).astype(np.float32).reshape(-1))
    out = dict(x=np.concatenate(xs), dg=np.concatenate(dgs), boxes=np.concatenate(bs), params=_params(case, rng))
    _INPUTS[key] = out
    return out


def embed64(p, dv, dg, e_dv):
    """float64 D_embed on (dv, dg) and the bound of the kernel's z against it -> (a, e_a)."""
    g = gamma_u
    if "w" in p:
        wv, wg, b = float(p["w"][0]), float(p["w"][1]), float(p["b"])
        z = wv * dv + wg * dg + b
        e_z = abs(wv) * e_dv + g(2) * (abs(wv) * (np.abs(dv) + e_dv) + np.abs(wg * dg) + abs(b))
    else:
        w1, b1, w2, b2 = (np.asarray(p[k], np.float64) for k in ("w1", "b1", "w2", "b2"))
        h = w1.shape[0]
        z, e_sum, mag = np.full_like(dv, float(b2)), np.zeros_like(dv), np.full_like(dv, abs(float(b2)))
        for k in range(h):
            pre = w1[k, 0] * dv + w1[k, 1] * dg + b1[k]
            e_k = abs(w1[k, 0]) * e_dv + g(2) * (abs(w1[k, 0]) * (np.abs(dv) + e_dv) + np.abs(w1[k, 1] * dg) + abs(b1[k]))
            hk = np.maximum(pre, 0.0)
            z = z + w2[k] * hk
            e_sum = e_sum + abs(w2[k]) * e_k
            mag = mag + abs(w2[k]) * (hk + e_k)
        e_z = e_sum + g(h) * mag
    with np.errstate(over="ignore"):
        a = 1.0 / (1.0 + np.exp(-z))
    return a, e_z / 4 + 3 * U32 + 2.0 ** -149


def worst_case_value_bound(d_embed, D):
    """The value bound of one adjacency entry for a model's own D_embed (nn.Sequential) and rows of width D, evaluated at the
    worst case |Dv| <= 1, |Dg| <= 1 and sum_d |x_id x_jd| <= |x_i| |x_j| (Cauchy-Schwarz): the expressions of the module
    docstring with those magnitudes.  For comparisons of whole-model outputs, where no float64 reference of the rows exists."""
    p = [t.detach().double().cpu().numpy() for t in d_embed.parameters()]
    g = gamma_u
    e_dv = (g(D) + 2 * (g(D) / (2 * (1 - g(D))) + U32) + 2 * U32) * (1 + 2.0 ** -10)
    if len(p) == 2:
        e_z = abs(p[0][0, 0]) * e_dv + g(2) * (abs(p[0][0, 0]) * (1 + e_dv) + abs(p[0][0, 1]) + abs(p[1][0]))
    else:
        h = p[0].shape[0]
        e_k = np.abs(p[0][:, 0]) * e_dv + g(2) * (np.abs(p[0][:, 0]) * (1 + e_dv) + np.abs(p[0][:, 1]) + np.abs(p[1]))
        h_k = np.abs(p[0]).sum(1) + np.abs(p[1])
        e_z = (np.abs(p[2][0]) * e_k).sum() + g(h) * (abs(p[3][0]) + (np.abs(p[2][0]) * (h_k + e_k)).sum())
    return float(e_z / 4 + 3 * U32)


def margin_rows(A, counts, bound):
    """Per scene, the rows of the valid block of A (S, mnp, mnp; anything numpy can read) whose every off-diagonal entry is
    farther from 0.5 than 4 x bound."""
    ok = []
    for s, n in enumerate(counts):
        a = np.asarray(A[s], np.float64)[:n, :n]
        clear = np.abs(a - 0.5) - 4 * bound
        np.fill_diagonal(clear, np.inf)
        ok.append((clear > 0).all(1))
    return ok


_REFS = {}


def reference(case):
    """float64 reference of one case, computed once and shared: dict(A, A_bound (S, mnp, mnp); gid (S, mnp) int64, -1 padded;
    sg (rows, D); colmax (S, D); card_sum, card_sum_bound (S); row_ok (rows,) bool: the whole adjacency row of that actor keeps
    the margin 4 x bound around 0.5; min_clear: the smallest (|a - 0.5| - margin) over all off-diagonal entries)."""
    key = case_id(case)
    if key in _REFS:
        return _REFS[key]
    inp = inputs(case)
    counts, D, mnp = case["counts"], case["D"], case["mnp"]
    so, do, _ = SC.offsets(counts)
    S = len(counts)
    out = dict(A=np.zeros((S, mnp, mnp)), A_bound=np.zeros((S, mnp, mnp)), gid=np.full((S, mnp), -1, np.int64),
               sg=np.zeros(inp["x"].shape), colmax=np.zeros((S, D)), card_sum=np.zeros(S), card_sum_bound=np.zeros(S),
               row_ok=np.zeros(sum(counts), bool), min_clear=np.inf)
    for s, n in enumerate(counts):
        x = inp["x"][so[s]:so[s] + n].astype(np.float64)
        dg = inp["dg"][do[s]:do[s] + n * n].astype(np.float64).reshape(n, n)
        nrm = np.sqrt((x * x).sum(1))
        nn_ = nrm[:, None] * nrm[None, :]
        dv = (x @ x.T) / nn_
        r_n = gamma_u(D) / (2 * (1 - gamma_u(D))) + U32
        e_dv = (gamma_u(D) * (np.abs(x) @ np.abs(x).T) / nn_ + np.abs(dv) * (2 * r_n + 2 * U32)) * (1 + 2.0 ** -10)
        a, e_a = embed64(inp["params"], dv, dg, e_dv)
        np.fill_diagonal(a, 1.0); e_a = e_a.copy(); np.fill_diagonal(e_a, 0.0)
        out["A"][s, :n, :n], out["A_bound"][s, :n, :n] = a, e_a
        off = ~np.eye(n, dtype=bool)
        clear = np.where(off, np.abs(a - 0.5) - 4 * e_a, np.inf)
        out["row_ok"][so[s]:so[s] + n] = (clear > 0).all(1)
        out["min_clear"] = min(out["min_clear"], float(clear.min()))
        gid = np.argmax(a >= 0.5, axis=1)                               # the first hit; the diagonal guarantees one
        out["gid"][s, :n] = gid
        for i in range(n):
            out["sg"][so[s] + i] = x[gid == gid[i]].max(0)
        out["colmax"][s] = x.max(0)
        out["card_sum"][s] = a.sum()
        out["card_sum_bound"][s] = e_a.sum() + gamma_u(2 * n) * (np.abs(a) + e_a).sum()
    _REFS[key] = out
    return out


def literal_per_scene(case):
    """forward_per_scene's eval-mode lines between _fuse and the heads, written out in torch float64 with the model's own
    helpers -> per scene (A_theta, group_id, pooled, card_feature)."""
    from multimodal_gar_amd.metric_ops import pairwise_cosine_similarity
    from multimodal_gar_amd.model.gat_model import GAR_Fusion_Net3
    inp = inputs(case)
    so, do, _ = SC.offsets(case["counts"])
    d_embed = make_d_embed(inp["params"]).double()
    outs = []
    with torch.no_grad():
        for s, n in enumerate(case["counts"]):
            fused = torch.from_numpy(inp["x"][so[s]:so[s] + n]).double()
            Dg = torch.from_numpy(inp["dg"][do[s]:do[s] + n * n]).double().view(n, n)
            Dv = pairwise_cosine_similarity(fused, zero_diagonal=False)
            feat = torch.cat((Dv.unsqueeze(-1), Dg.unsqueeze(-1)), dim=-1).reshape(-1, 2)
            A_theta = d_embed(feat).reshape(n, n).fill_diagonal_(1.)
            group_id = GAR_Fusion_Net3._predicted_groups(None, A_theta)
            pooled = GAR_Fusion_Net3._group_max_pool(fused, group_id)
            card = torch.cat((fused.max(dim=0, keepdim=True)[0], A_theta.sum().reshape([1, 1])), dim=1)
            outs.append((A_theta, group_id, pooled, card))
    return outs
