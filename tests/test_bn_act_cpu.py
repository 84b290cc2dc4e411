"""The float64 references and the bounds behind tests/test_bn_act_gpu.py (csrc/bn_act.hip), checked with no kernel:
the references are torch's BatchNorm -> ReLU -> max chain in float64, forward and through autograd; an fp32 numpy restatement
of each kernel's summation shape lies inside every bound on every case (the bounds are satisfiable, and every ReLU case keeps
its pre-activations off 0 by more than twice the forward bound); a deliberately wrong restatement leaves a bound (they bite);
and the host-side rejections return their codes through the C API without a device."""
import numpy as np
import pytest
import torch

import bn_act_cases as BC
import torch_refs as R

EPS = BC.EPS
f32 = np.float32
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
P1 = 0x1000   # a non-null pointer that a check must never dereference


def inside(got, want, bound):
    return bool((np.abs(np.asarray(got, np.float64) - want) <= bound).all())


# ------------------------------------------------------------------------------------------------ the kernels' shapes in fp32
def block_sum(v):
    """(..., 256) fp32 -> (...): a six-level tree over the 64 lanes of each wave, then the four waves in order."""
    w = v.reshape(v.shape[:-1] + (4, 64))
    while w.shape[-1] > 1:
        h = w.shape[-1] // 2
        w = w[..., :h] + w[..., h:]
    w = w[..., 0]
    t = np.zeros(w.shape[:-1], f32)
    for i in range(4):
        t = t + w[..., i]
    return t


def lanes(v, vec):
    """(C, nk) fp32 -> (C, L, 256[, 4]) in the kernel's lane order, zero-padded (adding 0 is exact)."""
    C, nk = v.shape
    per = 1024 if vec else 256
    L = -(-nk // per)
    v = np.concatenate([v, np.zeros((C, L * per - nk), f32)], 1)
    return v.reshape((C, L, 256, 4) if vec else (C, L, 256))


def emu_partials(xc, chunk, vec, sum_of_squares=False):
    """bn_partial_kernel: (cnt (K), chunk mean, chunk M2 (C, K) fp32)."""
    C, n = xc.shape
    cnt, means, m2s = [], [], []
    for e0 in range(0, n, chunk):
        v = xc[:, e0:e0 + chunk]
        nk = v.shape[1]
        npiv = min(256, nk)
        pv = np.concatenate([v[:, :npiv], np.zeros((C, 256 - npiv), f32)], 1)
        pivot = np.zeros(C, f32) if sum_of_squares else block_sum(pv) / f32(npiv)
        d = lanes(v - pivot[:, None], vec)
        s, q = np.zeros((C, 256), f32), np.zeros((C, 256), f32)
        for it in range(d.shape[1]):
            t = d[:, it]
            if vec:
                s = s + ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3]))
                q = q + ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + (t[..., 2] * t[..., 2] + t[..., 3] * t[..., 3]))
            else:
                s = s + t
                q = q + t * t
        sd, qd = block_sum(s).astype(np.float64), block_sum(q).astype(np.float64)
        cnt.append(float(nk))
        means.append((pivot.astype(np.float64) + sd / nk).astype(f32))
        m2s.append(np.maximum(qd - sd * sd / nk, 0.0).astype(f32))
    return np.array(cnt), np.stack(means, 1), np.stack(m2s, 1)


def emu_finalize(cnt, mean_k, m2_k, drop_last=False):
    """bn_finalize_kernel: the merge in double, mean / invstd rounded once; -> (mean fp32, invstd fp32, var float64)."""
    n = cnt.sum()
    if drop_last and len(cnt) > 1:
        cnt, mean_k, m2_k = cnt[:-1], mean_k[:, :-1], m2_k[:, :-1]
    mean_k, m2_k = mean_k.astype(np.float64), m2_k.astype(np.float64)
    m = (cnt * mean_k).sum(1) / n
    var = np.maximum((m2_k + cnt * (mean_k - m[:, None]) ** 2).sum(1) / n, 0.0)
    return m.astype(f32), (1.0 / np.sqrt(var + EPS)).astype(f32), var


def emu_stats(x, **wrong):
    B, C, P = x.shape
    xc = R.bn_channel_major(x).astype(f32)
    drop = wrong.pop("drop_last", False)
    return emu_finalize(*emu_partials(xc, R.bn_chunk(B, C, P), P % 4 == 0, **wrong), drop_last=drop)


def emu_running(means, variances, n, momentum, rm, rv, order=None, biased=False):
    """The fp32 momentum updates of bn_finalize_kernel / bn_running_update_grouped_kernel, rows in `order`."""
    mom, om = f32(momentum), f32(1.0) - f32(momentum)
    rm, rv = rm.astype(f32), rv.astype(f32)
    for g in (range(means.shape[0]) if order is None else order):
        rm = om * rm + mom * means[g].astype(f32)
        v = variances[g].astype(np.float64)
        rv = om * rv + mom * (v * n / (n - 1.0) if n > 1 and not biased else v).astype(f32)
    return rm, rv


def emu_apply(x, mean, invstd, gamma, beta, relu, per_sample=False):
    B, C, P = x.shape
    shp = (B, C, 1) if per_sample else (1, C, 1)
    g = np.ones(C, f32) if gamma is None else gamma
    b = np.zeros(C, f32) if beta is None else beta
    sc = invstd.astype(f32).reshape(shp) * g.reshape(1, C, 1)
    y = (x - mean.astype(f32).reshape(shp)) * sc + b.reshape(1, C, 1)
    return np.maximum(y, f32(0)) if relu else y


def emu_small(x, per_sample):
    """bn_small_fused_kernel's statistics: plain fp32 sum for the mean, two-pass M2 about it."""
    B, C, P = x.shape
    xc = (x.reshape(B * C, P) if per_sample else R.bn_channel_major(x).astype(f32)).astype(f32)
    n = xc.shape[1]
    d = lanes(xc, True)
    s = np.zeros((xc.shape[0], 256), f32)
    for it in range(d.shape[1]):
        t = d[:, it]
        s = s + ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3]))
    mu = block_sum(s) / f32(n)
    live = lanes(np.ones_like(xc), True)
    d = (d - mu[:, None, None, None]) * live
    q = np.zeros_like(s)
    for it in range(d.shape[1]):
        t = d[:, it]
        q = q + ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + (t[..., 2] * t[..., 2] + t[..., 3] * t[..., 3]))
    var = np.maximum(block_sum(q) / f32(n), f32(0))
    return mu, (1.0 / np.sqrt(var.astype(np.float64) + EPS)).astype(f32), var


def emu_bwd(dz, x, mean, invstd, gamma, chunk, vec, n=None):
    """bn_bwd_partial_kernel + bn_bwd_finalize_kernel + bn_bwd_apply_kernel on dz = the masked gradient (fp32)."""
    B, C, P = x.shape
    n = B * P if n is None else n
    g = np.ones(C, f32) if gamma is None else gamma
    mu, inv = mean.reshape(1, C, 1), invstd.reshape(1, C, 1)
    xh = (x - mu) * inv
    t1, t2 = R.bn_channel_major(dz).astype(f32), R.bn_channel_major(dz * xh).astype(f32)
    sums = []
    for t in (t1, t2):
        tot = np.zeros(C, np.float64)
        for e0 in range(0, t.shape[1], chunk):
            d = lanes(t[:, e0:e0 + chunk], vec)
            s = np.zeros((C, 256), f32)
            for it in range(d.shape[1]):
                for w in range(4 if vec else 1):
                    s = s + (d[:, it, :, w] if vec else d[:, it])
            tot += block_sum(s).astype(np.float64)
        sums.append(tot)
    dbeta, dgamma = sums[0].astype(f32), sums[1].astype(f32)
    m0, m1 = (sums[0] / n).astype(f32).reshape(1, C, 1), (sums[1] / n).astype(f32).reshape(1, C, 1)
    k = inv * g.reshape(1, C, 1)
    return dgamma, dbeta, np.stack([m0.ravel(), m1.ravel()], 1), k * (dz - m0 - xh * m1)


# ------------------------------------------------------------------------------------------------ the references are torch's
def test_references_are_torch_batchnorm_relu_max_in_float64():
    torch.manual_seed(0)
    B, C, M, ns = 3, 4, 5, 6
    x = torch.randn(B, C, M * ns, dtype=torch.float64) * 2 + 0.7
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([1.3, -0.7, 0.0, 0.9]))
        bn.bias.copy_(torch.tensor([0.2, -0.1, 0.5, -1.0]))
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    xt = x.clone().requires_grad_(True)
    pooled = torch.relu(bn(xt)).view(B, C, M, ns).max(dim=-1).values
    up = torch.randn(B, M, C, dtype=torch.float64).transpose(1, 2)          # a non-contiguous upstream gradient
    pooled.backward(up)
    mean, var = R.bn_stats_ref(x.numpy())
    invstd = (var + EPS) ** -0.5
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    pre, y, _ = R.bn_apply_ref(x.numpy(), mean, invstd, gamma, beta, 1)
    want, arg = R.bn_max_ref(pre.reshape(B, C, M, ns), 1)
    assert np.allclose(want, pooled.detach().numpy(), rtol=0, atol=1e-12)
    rm, rv, _, _ = R.bn_running_ref(mean, var, B * M * ns, 0.1, rm0, rv0)
    assert np.allclose(rm, bn.running_mean.numpy(), rtol=0, atol=1e-7) and np.allclose(rv, bn.running_var.numpy(), rtol=0, atol=1e-7)
    assert int(bn.num_batches_tracked) == 1
    d = up.numpy() * (want > 0)
    dz = np.zeros((B, C, M, ns))
    np.put_along_axis(dz, arg[..., None], d[..., None], -1)
    r = R.bn_bwd_ref(dz.reshape(B, C, M * ns), x.numpy(), mean, invstd, gamma)
    assert np.allclose(r["dx"], xt.grad.numpy(), rtol=0, atol=1e-11)
    assert np.allclose(r["dgamma"], bn.weight.grad.numpy(), rtol=0, atol=1e-11)
    assert np.allclose(r["dbeta"], bn.bias.grad.numpy(), rtol=0, atol=1e-11)
    # without the max: BatchNorm2d -> ReLU, dense gradient
    bn2 = torch.nn.BatchNorm2d(C, eps=EPS).double()
    x4 = x.view(B, C, M, ns).clone().requires_grad_(True)
    dy = torch.randn(B, C, M, ns, dtype=torch.float64)
    torch.relu(bn2(x4)).backward(dy)
    pre, y, _ = R.bn_apply_ref(x.numpy(), mean, invstd, None, None, 1)
    r = R.bn_bwd_ref(dy.numpy().reshape(B, C, -1) * (pre > 0), x.numpy(), mean, invstd, None)
    assert np.allclose(r["dx"].reshape(B, C, M, ns), x4.grad.numpy(), rtol=0, atol=1e-11)
    # Chan's merge of chunk partials is the direct variance
    xc = R.bn_channel_major(x.numpy())
    parts = [xc[:, i:i + 7] for i in range(0, xc.shape[1], 7)]
    m, m2 = R.bn_chan_merge_ref([p.shape[1] for p in parts], np.stack([p.mean(1) for p in parts], 1),
                                np.stack([((p - p.mean(1, keepdims=True)) ** 2).sum(1) for p in parts], 1))
    assert np.allclose(m, mean, rtol=0, atol=1e-12) and np.allclose(m2 / xc.shape[1], var, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ statistics
SMALLER_STATS = [n for n in sorted(BC.STATS_CASES) if n != "chunk_32768"]


@pytest.mark.parametrize("name", sorted(BC.STATS_CASES))
def test_kernel_shaped_statistics_are_inside_the_bounds(name):
    k = BC.stats_case(name)
    x = k["x"]
    mean, var, bmean, binv, bvar = R.bn_train_stats_bounds(x, EPS)
    m, i, v = emu_stats(x)
    assert inside(m, mean, bmean) and inside(i, (var + EPS) ** -0.5, binv) and inside(v, var, bvar + 1e-300)
    n = k["B"] * k["P"]
    for momentum in BC.MOMENTA:
        rm, rv, brm, brv = R.bn_running_ref(mean, var, n, momentum, k["running_mean"], k["running_var"], bmean, bvar)
        gm, gv = emu_running(m[None], v[None], n, momentum, k["running_mean"], k["running_var"])
        assert inside(gm, rm, brm) and inside(gv, rv, brv)
        if n > 1 and name != "chunk_32768":                    # n instead of n - 1 in the running variance
            gm, gv = emu_running(m[None], v[None], n, momentum, k["running_mean"], k["running_var"], biased=True)
            assert not inside(gv, rv, brv), name
    if name == "n1":
        assert (var == 0).all() and (v == 0).all()


def test_statistics_bounds_see_sum_of_squares_and_a_dropped_chunk():
    x = BC.stats_case("cancellation_mean1e4")["x"]
    mean, var, bmean, binv, _ = R.bn_train_stats_bounds(x, EPS)
    assert (np.abs(mean) > 5e3 * np.sqrt(var)).all()
    assert (binv < 1e-4 * (var + EPS) ** -0.5).all()           # the bound does not grow with |mean| / std = 1e4
    _, i, _ = emu_stats(x, sum_of_squares=True)
    assert not inside(i, (var + EPS) ** -0.5, binv)
    for name in ("second_chunk_of_4", "scalar_last_chunk_of_1", "vec_chunk_starts_inside_sample"):
        x = BC.stats_case(name)["x"]
        mean, var, bmean, binv, _ = R.bn_train_stats_bounds(x, EPS)
        m, i, _ = emu_stats(x, drop_last=True)
        assert not inside(m, mean, bmean), name


@pytest.mark.parametrize("name", sorted(BC.GROUPED_CASES))
def test_grouped_update_is_in_sample_order_and_the_bound_sees_any_other(name):
    k = BC.grouped_case(name)
    G, C, P = k["B"], k["C"], k["P"]
    mean, var, bmean, binv, bvar = R.bn_train_stats_bounds(k["x"].reshape(1, G * C, P), EPS)
    m, i, v = emu_stats(k["x"].reshape(1, G * C, P))
    assert inside(m, mean, bmean) and inside(i, (var + EPS) ** -0.5, binv)
    sh = (G, C)
    for momentum in BC.MOMENTA:
        rm, rv, brm, brv = R.bn_running_ref(mean.reshape(sh), var.reshape(sh), P, momentum, k["running_mean"], k["running_var"],
                                            bmean.reshape(sh), bvar.reshape(sh))
        gm, gv = emu_running(m.reshape(sh), v.reshape(sh), P, momentum, k["running_mean"], k["running_var"])
        assert inside(gm, rm, brm) and inside(gv, rv, brv)
        gm, gv = emu_running(m.reshape(sh), v.reshape(sh), P, momentum, k["running_mean"], k["running_var"], order=range(G - 1, -1, -1))
        assert not inside(gm, rm, brm) and not inside(gv, rv, brv)


# ------------------------------------------------------------------------------------------------ apply, small
@pytest.mark.parametrize("P", BC.APPLY_P)
def test_fp32_apply_is_inside_the_bound_and_relu_cases_are_off_the_threshold(P):
    for which in BC.APPLY_AFFINE:
        for per in (0, 1):
            for relu, mean in ((1, 0.7), (0, 0.7), (1, 1e4)):
                k = BC.apply_case(P, which, per, mean=mean, relu=bool(relu))
                pre, want, bound = R.bn_apply_ref(k["x"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per)
                if relu:
                    assert (np.abs(pre) > 2.0 * bound).all()
                else:
                    assert (np.abs(pre) <= np.abs(0 if k["beta"] is None else k["beta"]).max() + 1e-6).any()   # the near-zero values
                assert inside(emu_apply(k["x"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per), want, bound)
                assert bound.max() < 1e-5                         # also at mean 1e4: no |mean| term
    k = BC.apply_case(4100, "both", 0, mean=1e4)
    g, b = k["gamma"], k["beta"]
    sc = k["invstd"] * g
    folded = k["x"] * sc.reshape(1, -1, 1) + (b - k["mean"] * sc).reshape(1, -1, 1)        # x * sc + (beta - mean * sc)
    pre, want, bound = R.bn_apply_ref(k["x"], k["mean"], k["invstd"], g, b, 0)
    assert not inside(folded, pre, bound)


@pytest.mark.parametrize("name", sorted(BC.SMALL_CASES))
def test_small_kernel_shape_is_inside_the_train_stats_bounds(name):
    k = BC.small_case(name)
    B, C, P, per = k["B"], k["C"], k["P"], k["per_sample"]
    xs = k["x"].reshape(1, B * C, P) if per else k["x"]
    mean, var, bmean, binv, bvar = R.bn_train_stats_bounds(xs, EPS)
    mu, inv, v = emu_small(k["x"], per)
    assert inside(mu, mean, bmean) and inside(inv, (var + EPS) ** -0.5, binv)
    m2, _, _ = emu_stats(xs)
    assert inside(m2, mu.astype(np.float64), 2.0 * bmean)
    pre, want, bound = R.bn_apply_ref(k["x"], mu, inv, k["gamma"], k["beta"], 1, per)
    assert (np.abs(pre) > 2.0 * bound).all()
    assert inside(emu_apply(k["x"], mu, inv, k["gamma"], k["beta"], 1, per), want, bound)


# ------------------------------------------------------------------------------------------------ max
@pytest.mark.parametrize("ns", BC.TIE_NS)
def test_first_arg_max_on_ties_and_the_check_sees_the_last(ns):
    k = BC.tie_case(ns)
    B, C, M = k["B"], k["C"], k["M"]
    pre, _, bound = R.bn_apply_ref(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    pre, bound = pre.reshape(B, C, M, ns), bound.reshape(B, C, M, ns)
    assert (np.abs(pre) > 2.0 * bound).all() and (pre[:, 3] < 0).all()
    act = emu_apply(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 0).reshape(B, C, M, ns)
    first = np.argmax(act, -1)
    last = ns - 1 - np.argmax(act[..., ::-1], -1)
    want = np.broadcast_to(k["ties"][None, None], first.shape)
    assert (first[:, [0, 1, 3]] == want[:, [0, 1, 3]]).all() and (first[:, 2] == 0).all()
    assert (last[:, [0, 1, 3]] != want[:, [0, 1, 3]]).all() and (last[:, 2] == ns - 1).all()
    _, arg = R.bn_max_ref(pre, 1)
    assert (arg[:, [0, 1, 3]] == want[:, [0, 1, 3]]).all()
    if ns > 3:                                                 # the tied maximum beats every other slot by far more than the bound
        assert (pre.max(-1)[:, [0, 1, 3]] - np.sort(pre, -1)[..., -4][:, [0, 1, 3]] > 100 * bound.max()).all()


@pytest.mark.parametrize("name", sorted(BC.MAX_CASES))
def test_max_cases_are_off_the_threshold(name):
    k = BC.max_case(name)
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    pre, _, bound = R.bn_apply_ref(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    assert (np.abs(pre) > 2.0 * bound).all() and (pre[:, 3] < 0).all() and (pre[:, 0] > 0).any()
    act = emu_apply(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 1).reshape(B, C, M, ns)
    want, _ = R.bn_max_ref(pre.reshape(B, C, M, ns), 1)
    assert inside(act.max(-1), want, bound.reshape(B, C, M, ns).max(-1))


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("name", sorted(BC.BWD_CASES) + ["rowmajor_p65_c64"])
def test_kernel_shaped_backward_is_inside_the_bounds(name, relu):
    B, C, P = BC.BWD_CASES[name] if name in BC.BWD_CASES else (2, 64, 65)
    k = BC.bwd_case(B, C, P, relu)
    pre, _, bound = R.bn_apply_ref(k["x"], k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()
    mask = (pre > 0) if relu else np.ones_like(pre, bool)
    r = R.bn_bwd_ref(k["dy"] * mask, k["x"], k["mean"], k["invstd"], k["gamma"])
    chunk, vec = R.bn_chunk(B, C, P), P % 4 == 0
    nk = min(chunk, B * P)
    bbeta, bgamma, bcoef, bdx = R.bn_bwd_bounds(r, 4 * -(-nk // 1024) if vec else -(-nk // 256))
    dgamma, dbeta, coef, dx = emu_bwd((k["dy"] * mask).astype(f32), k["x"], k["mean"], k["invstd"], k["gamma"], chunk, vec)
    assert inside(dgamma, r["dgamma"], bgamma) and inside(dbeta, r["dbeta"], bbeta)
    assert inside(coef, r["coef"], bcoef) and inside(dx, r["dx"], bdx)
    # a dropped last chunk / the wrong mask leave the bounds
    if B * P % chunk and B * P > chunk:
        cut = (B * P // chunk) * chunk
        dzc = R.bn_channel_major(k["dy"] * mask)
        assert not inside(dzc[:, :cut].sum(1), r["dbeta"], bbeta)
    if relu and B * P > 1:
        r0 = R.bn_bwd_ref(k["dy"], k["x"], k["mean"], k["invstd"], k["gamma"])
        assert not inside(r0["dx"], r["dx"], bdx)


@pytest.mark.parametrize("ns", BC.MAXBWD_NS)
def test_kernel_shaped_maxpool_backward_is_inside_the_bounds(ns):
    k = BC.maxbwd_case(ns)
    B, C, M = k["B"], k["C"], k["M"]
    x3 = k["x"].reshape(B, C, M * ns)
    pre, _, bound = R.bn_apply_ref(x3, k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    assert (np.abs(pre) > 2.0 * bound).all()
    pooled, arg = R.bn_max_ref(pre.reshape(B, C, M, ns), 1)
    assert (pooled[:, 3] == 0).all() and (pooled[:, 0] > 0).any()
    d = k["dpool"] * (pooled > 0)
    dz = np.zeros((B, C, M, ns), f32)
    np.put_along_axis(dz, arg[..., None], d[..., None].astype(f32), -1)
    r = R.bn_bwd_ref(dz.reshape(B, C, M * ns), x3, k["mean"], k["invstd"], k["gamma"])
    chunk = R.bn_chunk(B, C, M)
    bbeta, bgamma, bcoef, bdx = R.bn_bwd_bounds(r, -(-min(chunk, B * M) // 256))
    # the reduction walks the B * M groups, one per lane and turn: the arg-max elements in (b, m) order
    da = np.take_along_axis(dz, arg[..., None], -1)[..., 0]
    xa = np.take_along_axis(k["x"], arg[..., None], -1)[..., 0]
    dgamma, dbeta, coef, _ = emu_bwd(da, xa, k["mean"], k["invstd"], k["gamma"], chunk, False, n=B * M * ns)
    assert inside(dgamma, r["dgamma"], bgamma) and inside(dbeta, r["dbeta"], bbeta) and inside(coef, r["coef"], bcoef)
    _, _, _, dx = emu_bwd(dz.reshape(B, C, M * ns), x3, k["mean"], k["invstd"], k["gamma"], 65536, False)
    assert inside(dx, r["dx"], bdx)


# ------------------------------------------------------------------------------------------------ partials
@pytest.mark.parametrize("name", sorted(BC.PARTIALS_CASES))
def test_partials_merge_in_double_is_inside_the_bounds_and_a_dropped_chunk_is_not(name):
    k = BC.partials_case(name)
    cnt, mean_k, m2_k = k["cnt"], k["partial"][:, :, 0], k["partial"][:, :, 1]
    mean, var, bmean, binv, _ = R.bn_from_partials_bounds(cnt, mean_k, m2_k, EPS)
    if k["merge"]:                                             # groups of 256 first, rounded to fp32
        gc, gm, gq = [], [], []
        for i in range(0, len(cnt), 256):
            m, q = R.bn_chan_merge_ref(cnt[i:i + 256], mean_k[:, i:i + 256], m2_k[:, i:i + 256])
            gc.append(cnt[i:i + 256].sum()), gm.append(m.astype(f32)), gq.append(q.astype(f32))
        cnt2, mk2, qk2 = np.array(gc), np.stack(gm, 1), np.stack(gq, 1)
        assert len(cnt2) == 5 and cnt2[-1] == 40
    else:
        cnt2, mk2, qk2 = cnt, mean_k, m2_k
    m, i, _ = emu_finalize(cnt2, mk2, qk2)
    assert inside(m, mean, bmean) and inside(i, (var + EPS) ** -0.5, binv)
    if len(cnt2) > 1:
        m, i, _ = emu_finalize(cnt2, mk2, qk2, drop_last=True)
        assert not inside(m, mean, bmean)


# ------------------------------------------------------------------------------------------------ host-side rejections
def _fn(name):
    from multimodal_gar_amd import _lib
    return _lib._fns[name], _lib._cdll.mgar_last_error


def test_host_side_rejections_return_their_codes_without_a_device():
    for entry in ("mgar_bn_act_small", "mgar_bn_act_small_bf16"):
        fn, err = _fn(entry)
        for B, C, P, per in BC.SMALL_REJECTED.values():
            assert fn(P1, B, C, P, per, EPS, 0.1, None, None, 1, None, None, None, None, None, None, P1, -1, None) == EUNSUPPORTED
            assert b"16384" in err()
        assert fn(P1, 0, 3, 1028, 0, EPS, 0.1, None, None, 1, None, None, None, None, None, None, P1, -1, None) == OK
    for entry in ("mgar_bn_act_maxpool_fwd", "mgar_bn_act_maxpool_fwd_bf16"):
        fn, err = _fn(entry)
        assert fn(P1, 1, 1, 1, 256, P1, P1, None, None, 1, P1, P1, None, None) == EINVAL and b"bad sizes" in err()
        assert fn(P1, 1, 1, 1, 0, P1, P1, None, None, 1, P1, P1, None, None) == EINVAL
        assert fn(P1, 1, 1, 0, 255, P1, P1, None, None, 1, P1, P1, None, None) == OK
    fn, err = _fn("mgar_bn_act_bwd_rowmajor")
    assert fn(P1, P1, 2, 65, 64, P1, P1, None, None, 1, P1, None, None, P1, None) == EUNSUPPORTED and b"C <= 64" in err()
    fn, err = _fn("mgar_bn_stats_from_partials")
    for nchunk, chunk, last, _ in BC.PARTIALS_CASES.values():
        n = (nchunk - 1) * chunk + last
        assert fn(P1, nchunk, 3, nchunk * chunk + 1, chunk, EPS, 0.1, None, P1, P1, None, None, None, None) == EINVAL
        assert b"cover" in err()
        assert fn(P1, nchunk + 1, 3, n, chunk, EPS, 0.1, None, P1, P1, None, None, None, None) == EINVAL
    ws, _ = _fn("mgar_bn_stats_from_partials_workspace_floats")
    assert ws(1, 3) == 0 and ws(1024, 3) == 0 and ws(1025, 3) == 2 * 3 * 5 and ws(-1, 3) == -1
    # the merge route without a workspace is rejected before any launch
    assert fn(P1, 1025, 3, 1024 * 128 + 40, 128, EPS, 0.1, None, P1, P1, None, None, None, None) == EINVAL and b"workspace" in err()
