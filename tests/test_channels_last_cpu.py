"""The float64 references and the bounds behind tests/test_channels_last_ops_gpu.py and tests/test_maxpool3d_gpu.py
(csrc/channels_last.hpp, csrc/maxpool3d.hip), checked with no kernel: the references are torch's BatchNorm -> ReLU and
F.pad -> max_pool3d chains in float64; an fp32 numpy restatement of each kernel's summation shape (row lanes, the lanes added
in order, the first-row pivot, the finish in double) lies inside every bound on every case; deliberately wrong restatements
leave a bound (they bite); every ReLU case keeps its pre-activations off 0 by more than twice the forward bound; and the
host-side rejections return their codes through the C API without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import channels_last_cases as CC
import torch_refs as R
from test_bn_act_cpu import emu_apply, emu_finalize, emu_running, inside

EPS = CC.EPS
f32 = np.float32
OK, EINVAL = 0, -1
P1 = 0x1000   # a non-null, 16-byte aligned pointer that a check must never dereference


# ------------------------------------------------------------------------------------------------ the kernels' shapes in fp32
def lane_sums(terms, rpar, drop_lane=False):
    """terms (K, nk, C) fp32, the per-row terms of K chunks -> (K, C) fp32: row lane rr adds rows rr, rr + rpar, ... in order,
    then lane 0 adds lanes 1 .. rpar - 1 in order (padding rows are zeros: adding 0 is exact)."""
    K, nk, C = terms.shape
    L = -(-nk // rpar)
    t = np.concatenate([terms, np.zeros((K, L * rpar - nk, C), f32)], 1).reshape(K, L, rpar, C)
    s = np.zeros((K, rpar, C), f32)
    for it in range(L):
        s = s + t[:, it]
    tot = s[:, 0]
    for q in range(1, rpar - (1 if drop_lane else 0)):
        tot = tot + s[:, q]
    return tot


def chunk_groups(xr, chunk):
    """The chunks of the rows xr (rows, C) as arrays (K, nk, C) of equal nk: the full ones, then the ragged last one."""
    rows, C = xr.shape
    full = rows // chunk
    if full:
        yield xr[:full * chunk].reshape(full, chunk, C)
    if rows % chunk:
        yield xr[None, full * chunk:]


def emu_cl_partials(xr, chunk, drop_lane=False):
    """bn_cl_partial_kernel on the rows (rows, C) fp32 of one statistics group: (cnt (K), chunk mean, chunk M2 (C, K) fp32)."""
    C = xr.shape[1]
    rpar = R.CL_THREADS // (C // 4)
    cnt, means, m2s = [], [], []
    for v in chunk_groups(xr, chunk):
        nk = v.shape[1]
        piv = v[:, 0]
        d = v - piv[:, None]
        sd = lane_sums(d, rpar, drop_lane).astype(np.float64)
        qd = lane_sums(d * d, rpar, drop_lane).astype(np.float64)
        cnt += [float(nk)] * v.shape[0]
        means.append((piv.astype(np.float64) + sd / nk).astype(f32))
        m2s.append(np.maximum(qd - sd * sd / nk, 0.0).astype(f32))
    return np.array(cnt), np.concatenate(means).T, np.concatenate(m2s).T


def emu_cl_stats(x, per_sample, drop_last=False, drop_lane=False):
    """mgar_bn_cl_train_stats on x (S, R, C) fp32 -> (mean fp32, invstd fp32, var float64), (C) or (S * C)."""
    S, Rr, C = x.shape
    if per_sample:
        chunk = R.bn_cl_chunk_rows(S, Rr)
        parts = [emu_finalize(*emu_cl_partials(x[s], chunk, drop_lane), drop_last=drop_last) for s in range(S)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    return emu_finalize(*emu_cl_partials(x.reshape(S * Rr, C), R.bn_cl_chunk_rows(1, S * Rr), drop_lane), drop_last=drop_last)


def emu_rows_bwd(dz, x, mean, invstd, gamma):
    """mgar_bn_rows_bwd on dz = the masked gradient, x (rows, C) fp32 -> (dgamma, dbeta, coef (C, 2), dx (rows, C)) fp32."""
    rows, C = x.shape
    rpar = R.CL_THREADS // (C // 4)
    chunk = R.bn_cl_chunk_rows(1, rows)
    g = np.ones(C, f32) if gamma is None else gamma
    xh = (x - mean[None]) * invstd[None]
    sums = []
    for t in (dz, dz * xh):
        sums.append(sum(lane_sums(v, rpar).astype(np.float64).sum(0) for v in chunk_groups(t.astype(f32), chunk)))
    dbeta, dgamma = sums[0].astype(f32), sums[1].astype(f32)
    m0, m1 = (sums[0] / rows).astype(f32), (sums[1] / rows).astype(f32)
    k = invstd * g
    return dgamma, dbeta, np.stack([m0, m1], 1), k[None] * (dz - m0[None] - (x - mean[None]) * invstd[None] * m1[None])


# ------------------------------------------------------------------------------------------------ the references are torch's
def test_references_are_torch_batchnorm_relu_in_float64():
    torch.manual_seed(0)
    S, Rr, C = 3, 10, 8
    x = torch.randn(S, Rr, C, dtype=torch.float64) * 2 + 0.7
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([1.3, -0.7, 0.0, 0.9, 1.1, 0.4, -1.2, 2.0]))
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    # all samples at once: BatchNorm1d over the S * R rows, ReLU, and its autograd backward
    xt = x.reshape(S * Rr, C).clone().requires_grad_(True)
    y = torch.relu(bn(xt))
    dy = torch.randn(S * Rr, C, dtype=torch.float64)
    y.backward(dy)
    mean, var, _, _, _ = R.bn_cl_train_stats_bounds(x.numpy(), 0, EPS)
    invstd = (var + EPS) ** -0.5
    xc = CC.to_bcp(x.numpy().reshape(1, S * Rr, C))
    pre, want, _ = R.bn_apply_ref(xc, mean, invstd, gamma, beta, 1)
    assert np.allclose(want[0].T, y.detach().numpy(), rtol=0, atol=1e-12)
    rm, rv, _, _ = R.bn_running_ref(mean, var, S * Rr, 0.1, rm0, rv0)
    assert np.allclose(rm, bn.running_mean.numpy(), rtol=0, atol=1e-7) and np.allclose(rv, bn.running_var.numpy(), rtol=0, atol=1e-7)
    r = R.bn_bwd_ref(CC.to_bcp(dy.numpy()[None]) * (pre > 0), xc, mean, invstd, gamma)
    assert np.allclose(r["dx"][0].T, xt.grad.numpy(), rtol=0, atol=1e-11)
    assert np.allclose(r["dgamma"], bn.weight.grad.numpy(), rtol=0, atol=1e-11)
    assert np.allclose(r["dbeta"], bn.bias.grad.numpy(), rtol=0, atol=1e-11)
    # per sample: the module is called once per sample, in sample order
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rm0)), bn.running_var.copy_(torch.from_numpy(rv0))
        ys = torch.stack([torch.relu(bn(x[s])) for s in range(S)])
    mean, var, _, _, _ = R.bn_cl_train_stats_bounds(x.numpy(), 1, EPS)
    _, want, _ = R.bn_apply_ref(CC.to_bcp(x.numpy()), mean, (var + EPS) ** -0.5, gamma, beta, 1, True)
    assert np.allclose(CC.to_rows(want), ys.numpy(), rtol=0, atol=1e-12)
    rm, rv, _, _ = R.bn_running_ref(mean.reshape(S, C), var.reshape(S, C), Rr, 0.1, rm0, rv0)
    # three updates with fp32(0.1) against torch's 0.1: 1.5e-8 relative each
    assert np.allclose(rm, bn.running_mean.numpy(), rtol=0, atol=5e-7) and np.allclose(rv, bn.running_var.numpy(), rtol=0, atol=5e-7)
    swapped = R.bn_running_ref(mean.reshape(S, C)[::-1], var.reshape(S, C)[::-1], Rr, 0.1, rm0, rv0)[0]
    assert not np.allclose(swapped, bn.running_mean.numpy(), rtol=0, atol=1e-3)
    # NCDHW in, NDHWC out: BatchNorm3d -> ReLU -> permute
    bn3 = torch.nn.BatchNorm3d(C, eps=EPS).double()
    x5 = x.permute(0, 2, 1).reshape(S, C, 1, 2, 5)
    y5 = torch.relu(bn3(x5)).permute(0, 2, 3, 4, 1).reshape(S, Rr, C)
    mean, var, _, _, _ = R.bn_cl_train_stats_bounds(x.numpy(), 0, EPS)
    _, want, _ = R.bn_apply_ref(CC.to_bcp(x.numpy()), mean, (var + EPS) ** -0.5, None, None, 1)
    assert np.allclose(CC.to_rows(want), y5.detach().numpy(), rtol=0, atol=1e-12)


def _torch_pool(x, k, s, pad_value):
    pads = [R.same_pads(x.shape[-3 + i], k[i], s[i]) for i in range(3)]
    xp = F.pad(torch.from_numpy(np.asarray(x, np.float64))[None], pads[2] + pads[1] + pads[0], value=pad_value)
    return F.max_pool3d(xp, k, s)[0].numpy()


@pytest.mark.parametrize("name", [n for n in sorted(CC.POOL_CASES) if CC.POOL_CASES[n]["NC"] <= 3])
def test_pool_reference_is_torch_pad_then_max_pool3d_and_cases_take_their_route(name):
    k = CC.pool_case(name)
    assert CC.pool_route(k["NC"], k["T"], k["H"], k["W"], k["k"], k["s"]) == k["route"]
    x = k["x"].copy()
    for pad_value in (0.0, -np.inf):
        want = R.maxpool3d_ref(x, k["k"], k["s"], pad_value)
        assert want.shape == (k["NC"],) + tuple(-(-n // st) for n, st in zip((k["T"], k["H"], k["W"]), k["s"]))
        assert np.array_equal(want, _torch_pool(x, k["k"], k["s"], pad_value))
        assert np.isfinite(want).all()                           # "valid": every window holds an element of the input
    same, valid = R.maxpool3d_ref(x, k["k"], k["s"], 0.0), R.maxpool3d_ref(x, k["k"], k["s"], -np.inf)
    if k["negative"]:
        touches = R.maxpool3d_ref(np.zeros_like(x), k["k"], k["s"], 1.0) > 0
        assert touches.any() and (same[touches] == 0).all() and (valid < 0).all()
    x[0, 0, 0, 0] = np.nan        # a NaN is the maximum of every window that holds it (a stride > kernel skips elements, never 0)
    want = R.maxpool3d_ref(x, k["k"], k["s"], 0.0)
    assert np.isnan(want).any() and np.array_equal(want, _torch_pool(x, k["k"], k["s"], 0.0), equal_nan=True)


def test_the_nc_65536_case_takes_the_scalar_route_and_nan_sites_exist():
    assert CC.pool_route(65536, 1, 1, 4, (3, 3, 3), (1, 1, 1)) == "scalar"
    assert CC.pool_route(65535, 1, 1, 4, (3, 3, 3), (1, 1, 1)) == "quad1"
    for name, (t, h, w), _ in CC.POOL_NAN_SITES:
        c = CC.POOL_CASES[name]
        assert t < c["T"] and h < c["H"] and w < c["W"]


def test_same_pool_of_relu_bn_equals_relu_bn_of_valid_pool_for_positive_gamma():
    rng = np.random.default_rng(5)
    C = 4
    x = rng.standard_normal((2, C, 4, 5, 8))
    mean, invstd = x.mean((0, 2, 3, 4)), x.var((0, 2, 3, 4)) ** -0.5
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    bn = lambda t: np.maximum((t - mean[None, :, None, None, None]) * (invstd * gamma)[None, :, None, None, None]   # noqa: E731
                              + beta[None, :, None, None, None], 0.0)
    for k, s in CC.POOL_CL_GEOMETRIES:
        assert np.array_equal(R.maxpool3d_ref(bn(x), k, s, 0.0), bn(R.maxpool3d_ref(x, k, s, -np.inf)))
    gamma[1] = -gamma[1]                                         # not for a negative gamma
    assert not np.array_equal(R.maxpool3d_ref(bn(x), (3, 3, 3), (1, 1, 1), 0.0), bn(R.maxpool3d_ref(x, (3, 3, 3), (1, 1, 1), -np.inf)))


def test_chunk_rows_restated():
    assert R.bn_cl_chunk_rows(1, 300) == 256 and R.bn_cl_chunk_rows(1, 7) == 7 and R.bn_cl_chunk_rows(1, 600000) == 293
    assert -(-600000 // 293) == 2048 and 600000 - 2047 * 293 == 229
    assert R.bn_cl_chunk_rows(3, 300) == 256 and R.bn_cl_chunk_rows(1, 257) == 256


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("name", sorted(CC.STATS_CASES))
def test_kernel_shaped_statistics_are_inside_the_bounds(name):
    k = CC.stats_case(name)
    S, Rr, C, per = k["S"], k["R"], k["C"], k["per_sample"]
    mean, var, bmean, binv, bvar = R.bn_cl_train_stats_bounds(k["x"], per, EPS)
    m, i, v = emu_cl_stats(k["x"], per)
    assert inside(m, mean, bmean) and inside(i, (var + EPS) ** -0.5, binv) and inside(v, var, bvar + 1e-300)
    G, n = (S, Rr) if per else (1, S * Rr)
    sh = (G, C)
    for momentum in CC.MOMENTA:
        rm, rv, brm, brv = R.bn_running_ref(mean.reshape(sh), var.reshape(sh), n, momentum, k["running_mean"], k["running_var"],
                                            bmean.reshape(sh), bvar.reshape(sh))
        gm, gv = emu_running(m.reshape(sh), v.reshape(sh), n, momentum, k["running_mean"], k["running_var"])
        assert inside(gm, rm, brm) and inside(gv, rv, brv)
        if per:                                                  # any other order of the three updates leaves the bound
            gm, gv = emu_running(m.reshape(sh), v.reshape(sh), n, momentum, k["running_mean"], k["running_var"],
                                 order=range(G - 1, -1, -1))
            assert not inside(gm, rm, brm) and not inside(gv, rv, brv)
        elif n > 1 and n < 10000 and name != "outlier_in_pivot_row":   # n instead of n - 1 in the running variance
            gm, gv = emu_running(m[None], v[None], n, momentum, k["running_mean"], k["running_var"], biased=True)
            assert not inside(gv, rv, brv), name
    if name == "one_row":
        assert (var == 0).all() and (v == 0).all() and (i == f32(1.0 / np.sqrt(EPS))).all()
    if name == "r257_last_chunk_of_1":
        assert (emu_cl_partials(k["x"][0], 256)[2][:, 1] == 0).all()


def test_statistics_bounds_see_a_dropped_chunk_a_dropped_row_lane_and_sum_of_squares():
    for name in ("c4_256_row_lanes", "r257_last_chunk_of_1", "s3_chunks_cross_samples", "per_sample_s3", "chunk_293"):
        k = CC.stats_case(name)
        mean, var, bmean, binv, _ = R.bn_cl_train_stats_bounds(k["x"], k["per_sample"], EPS)
        m, i, _ = emu_cl_stats(k["x"], k["per_sample"], drop_last=True)
        assert not inside(m, mean, bmean), name
    for name in ("c24_rpar42_4_idle", "c4_256_row_lanes", "r7_c16_fewer_rows_than_lanes"):      # rr = rpar - 1 never added
        k = CC.stats_case(name)
        rpar = R.CL_THREADS // (k["C"] // 4)
        mean, var, bmean, binv, _ = R.bn_cl_train_stats_bounds(k["x"], 0, EPS)
        m, i, _ = emu_cl_stats(k["x"], 0, drop_lane=True)
        assert inside(m, mean, bmean) == (k["R"] < rpar), name      # 7 rows: lane rpar - 1 holds none
    x = CC.stats_case("cancellation_mean1e4")["x"]
    mean, var, bmean, binv, _ = R.bn_cl_train_stats_bounds(x, 0, EPS)
    assert (np.abs(mean) > 5e3 * np.sqrt(var)).all()
    assert (binv < 1e-4 * (var + EPS) ** -0.5).all()               # the bound does not grow with |mean| / std = 1e4
    xr = x[0].astype(np.float64)
    s, q = xr.astype(f32).sum(0, dtype=f32), (xr.astype(f32) ** 2).sum(0, dtype=f32)    # E[x^2] - E[x]^2 in fp32
    v = np.maximum(q.astype(np.float64) / 300 - (s.astype(np.float64) / 300) ** 2, 0.0)
    assert not inside((v + EPS) ** -0.5, (var + EPS) ** -0.5, binv)


def test_outlier_in_the_pivot_row_keeps_a_usable_bound():
    """The figures quoted at the case in channels_last_cases.py."""
    import bn_act_cases as BC
    x = CC.stats_case("outlier_in_pivot_row")["x"]
    mean, var, bmean, binv, bvar = R.bn_cl_train_stats_bounds(x, 0, EPS)      # asserts low > 0 itself
    rel = (binv * (var + EPS) ** 0.5).max()
    xa = BC.stats_case("outlier_in_pivot")["x"]
    ma, va, _, bia, _ = R.bn_train_stats_bounds(xa, EPS)
    rel_a = (bia * (va + EPS) ** 0.5).max()
    print("invstd bound / invstd: channels-last %.3g, bn_act.hip %.3g; dvar / var %.3g" % (rel, rel_a, (bvar / var).max()))
    assert rel < 1e-2 and rel > 10 * rel_a


# ------------------------------------------------------------------------------------------------ apply
def _apply_cases():
    for C in CC.APPLY_C:
        for which in CC.APPLY_AFFINE:
            for per in (0, 1):
                for relu in (1, 0):
                    yield (3, 5, C, which, per, relu)
    for which in CC.APPLY_AFFINE:
        yield (1, 257, 4, which, 0, 1)


def test_fp32_apply_is_inside_the_bound_and_relu_cases_are_off_the_threshold():
    assert 257 * (4 // 4) % 256 == 1
    for S, Rr, C, which, per, relu in _apply_cases():
        k = CC.apply_case(S, Rr, C, which, per, bool(relu))
        pre, want, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per)
        if relu:
            assert (np.abs(pre) > 2.0 * bound).all()
        assert inside(emu_apply(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per), want, bound)
        assert np.array_equal(CC.to_bcp(k["x"]), k["xc"])
        if which == "both":
            assert k["gamma"][1] < 0 and k["gamma"][2] == 0
    for R_, C in ((r, c) for r in CC.TO_CL_R for c in CC.TO_CL_C):
        for per in (0, 1):
            k = CC.to_cl_case(R_, C, per)
            pre, want, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 1, per)
            assert (np.abs(pre) > 2.0 * bound).all()
            assert inside(emu_apply(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 1, per), want, bound)


def test_apply_bound_sees_the_per_sample_index_taken_without_times_c():
    """si = row / R + c instead of (row / R) * C + c: sample 0 is right, samples 1 and 2 read their neighbours' statistics."""
    for C in CC.APPLY_C:
        k = CC.apply_case(3, 5, C, "both", 1)
        S = 3
        pre, want, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 1, True)
        pad = np.concatenate([k["mean"], np.zeros(S, f32)]), np.concatenate([k["invstd"], np.ones(S, f32)])
        wrong = [np.stack([p[s:s + C] for s in range(S)]).reshape(-1) for p in pad]
        got = emu_apply(k["xc"], wrong[0], wrong[1], k["gamma"], k["beta"], 1, True)
        assert inside(got[0], want[0], bound[0]) and not inside(got[1], want[1], bound[1]) and not inside(got[2], want[2], bound[2])


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("which", ["both", "none"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("name", sorted(CC.BWD_CASES))
def test_kernel_shaped_backward_is_inside_the_bounds(name, relu, which):
    k = CC.bwd_case(name, relu, which)
    rows, C = k["rows"], k["C"]
    pre, _, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()
    mask = (pre > 0) if relu else np.ones_like(pre, bool)
    r = R.bn_bwd_ref(k["dyc"] * mask, k["xc"], k["mean"], k["invstd"], k["gamma"])
    bbeta, bgamma, bcoef, bdx = R.bn_bwd_bounds(r, R.bn_rows_bwd_lane_chain(rows, C))
    dgamma, dbeta, coef, dx = emu_rows_bwd((k["dy"] * mask[0].T).astype(f32), k["x"], k["mean"], k["invstd"], k["gamma"])
    assert inside(dgamma, r["dgamma"], bgamma) and inside(dbeta, r["dbeta"], bbeta)
    assert inside(coef, r["coef"], bcoef) and inside(dx, r["dx"][0].T, bdx[0].T)
    chunk = R.bn_cl_chunk_rows(1, rows)
    if rows > chunk:                                             # a dropped last chunk leaves the bound
        cut = ((rows - 1) // chunk) * chunk
        assert not inside((k["dyc"] * mask)[0, :, :cut].sum(1), r["dbeta"], bbeta)
    if relu and rows > 1:                                        # so does a gradient that ignores the mask
        r0 = R.bn_bwd_ref(k["dyc"], k["xc"], k["mean"], k["invstd"], k["gamma"])
        assert not inside(r0["dx"], r["dx"], bdx)


# ------------------------------------------------------------------------------------------------ host-side rejections
def _fn(name):
    from multimodal_gar_amd import _lib
    return _lib._fns[name], _lib._cdll.mgar_last_error


def test_host_side_rejections_return_their_codes_without_a_device():
    for sfx in ("", "_bf16"):
        stats, err = _fn("mgar_bn_cl_train_stats" + sfx)
        apply_, _ = _fn("mgar_bn_cl_act_fwd" + sfx)
        to_cl, _ = _fn("mgar_bn_act_fwd_to_cl" + sfx)
        pool_cl, _ = _fn("mgar_maxpool3d_same_fwd_cl" + sfx)
        esz = 4 if sfx == "" else 2
        for S, Rr, C in CC.CL_REJECTED_SHAPES.values():
            assert stats(P1, S, Rr, C, 0, EPS, 0.1, P1, P1, P1, None, None, None, None) == EINVAL and b"C % 4" in err()
            assert apply_(P1, S, Rr, C, 0, P1, P1, None, None, 1, P1, C, None) == EINVAL and b"C % 4" in err()
        S, Rr, C = CC.S_TIMES_C_TOO_LARGE
        assert S * C == 65536
        assert stats(P1, S, Rr, C, 1, EPS, 0.1, P1, P1, P1, None, None, None, None) == EINVAL and b"65535" in err()
        assert apply_(P1, 2, 8, 8, 0, P1, P1, None, None, 1, P1, 4, None) == EINVAL and b"ldy" in err()       # ldy < C
        assert apply_(P1, 2, 8, 8, 0, P1, P1, None, None, 1, P1, 10, None) == EINVAL and b"ldy" in err()      # ldy % 4 != 0
        assert apply_(P1, 2, 8, 8, 0, P1, P1, None, None, 1, P1 + esz, 8, None) == EINVAL and b"aligned" in err()
        assert apply_(None, 2, 8, 8, 0, P1, P1, None, None, 1, P1, 8, None) == EINVAL and b"null" in err()
        assert stats(None, 2, 8, 8, 0, EPS, 0.1, P1, P1, P1, None, None, None, None) == EINVAL and b"null" in err()
        assert to_cl(P1, 2, 8, 8, 0, P1, P1, None, None, 1, P1, 7, None) == EINVAL                            # ldy < C
        assert to_cl(None, 2, 8, 8, 0, P1, P1, None, None, 1, P1, 8, None) == EINVAL and b"null" in err()
        for S, Rr, C in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):          # empty shapes: OK with NULL pointers
            assert stats(None, S, Rr, C, 0, EPS, 0.1, None, None, None, None, None, None, None) == OK
            assert apply_(None, S, Rr, C, 0, None, None, None, None, 1, None, max(C, 4), None) == OK
            assert to_cl(None, S, C, Rr, 0, None, None, None, None, 1, None, C, None) == OK
        assert pool_cl(P1, 1, 2, 2, 2, 6, 3, 3, 3, 1, 1, 1, P1, None) == EINVAL and b"C % 4" in err()
        assert pool_cl(P1, 1, 2, 2, 2, 8, 0, 3, 3, 1, 1, 1, P1, None) == EINVAL and b"kernel / stride" in err()
        assert pool_cl(P1, 1, 2, 2, 2, 8, 3, 3, 3, 1, 0, 1, P1, None) == EINVAL
        assert pool_cl(None, 1, 2, 2, 2, 8, 3, 3, 3, 1, 1, 1, P1, None) == EINVAL and b"null" in err()
        assert pool_cl(None, 0, 2, 2, 2, 8, 3, 3, 3, 1, 1, 1, None, None) == OK
        for kind in ("same", "valid"):
            pool, _ = _fn("mgar_maxpool3d_%s_fwd%s" % (kind, sfx))
            assert pool(P1, 1, 2, 2, 2, 3, 3, 0, 1, 1, 1, P1, None) == EINVAL and b"bad sizes" in err()
            assert pool(P1, 1, 2, 2, 2, 3, 3, 3, 0, 1, 1, P1, None) == EINVAL
            assert pool(None, 1, 2, 2, 2, 3, 3, 3, 1, 1, 1, P1, None) == EINVAL and b"null" in err()
            assert pool(None, 0, 2, 2, 2, 3, 3, 3, 1, 1, 1, None, None) == OK
    ws, _ = _fn("mgar_bn_cl_workspace_floats")
    assert ws(1, 300, 4, 0) == 2 * 4 * 2 + 4 and ws(3, 300, 8, 1) == 2 * 3 * 8 * 2 + 24 and ws(3, 300, 8, 0) == 2 * 8 * 4 + 8
    assert ws(1, 600000, 4, 0) == 2 * 4 * 2048 + 4 and ws(1, 8, 6, 0) == 0 and ws(0, 8, 8, 0) == 0
    bwd, err = _fn("mgar_bn_rows_bwd")
    bws, _ = _fn("mgar_bn_rows_bwd_workspace_floats")
    assert bwd(P1, P1, 8, 6, P1, P1, None, None, 1, P1, None, None, P1, None) == EINVAL and b"C % 4" in err()
    assert bwd(P1, P1, 8, 1028, P1, P1, None, None, 1, P1, None, None, P1, None) == EINVAL
    assert bwd(None, P1, 8, 8, P1, P1, None, None, 1, P1, None, None, P1, None) == EINVAL and b"null" in err()
    assert bwd(None, None, 0, 8, None, None, None, None, 1, None, None, None, None, None) == OK
    assert bws(8, 6) == -1 and bws(257, 4) == 2 * 4 * 2 + 8 and bws(600000, 4) == 2 * 4 * 2048 + 8
