"""BatchNorm(train) + ReLU + max over nsample (csrc/bn_act.hip): every C entry point the header declares for that file, and
its bf16 twin where one exists, against the float64 references of torch_refs.py on the hand-built inputs of
bn_act_cases.py.  tests/test_bn_act_cpu.py shows, with no kernel, that the references are torch's BatchNorm chain, that the
bounds are satisfiable and that they bite.  The bounds are rounding counts, none is fitted to a
kernel's output.

Calls go through `_lib` with raw pointers.  dev(), nans(), guards_intact(), within() and same_bits() are those of
tests/test_query_group_gpu.py (imported, not copied): every input has 16 384 finite elements of slack behind it, every
output and every workspace (sized by the library's own size query) starts as payload NaNs with a guard behind that must keep
its bits, and every comparison logs the share of its bound that it used.  Every backward runs twice and must be bit-equal.

Which case covers which edge:
  statistics       second_chunk_of_4 (pivot from 4 lanes), scalar_last_chunk_of_1, odd_p_chunk_crosses_samples,
                   vec_chunk_starts_inside_sample, n1 (var 0, no unbiased correction), cancellation_mean1e4,
                   outlier_in_pivot, chunk_32768 (134 MB; momentum 0.1 only, it takes about as long as all others);
                   running_* / num_batches_tracked given and NULL, momentum 0.1 and 1.0; grouped G = 3 in sample order
  apply            P in {3, 4, 4096, 4097, 4100} x gamma / beta NULL in every combination, gamma < 0 and = 0, per-sample
                   statistics, y_bstride = C P + 8 with the gap keeping its bits, mean 1e4; without ReLU the near-zero values
  small fused      n = 4, 1 028, 16 384, per-sample B = 3 with running statistics, mean / invstd NULL, strided y, against
                   the two-call route; n = 16 388 and P % 4 != 0 rejected
  max-pool forward nsample 1..255 at M = 1, M one past a block (ns 4 / 64 / 5), exact ties per butterfly stage, gamma < 0,
                   gamma = 0, an all-negative channel under ReLU, xarg NULL / given, nsample 256 rejected
  backward         the statistics shapes, relu 0 / 1, gamma / beta NULL, row-major P in {63, 64, 65} x C in {1, 64} (65
                   rejected), apply-only with the test's float64 coef in both layouts
  max-pool backward nsample {3, 4, 5, 64, 255} x dpool contiguous / channel slice / transposed rows; _reduce with sc < 0 and
                   with explicit strides, dmask exactly dpool or 0; xarg NULL == xarg given bit for bit
  from partials    1 chunk, 1 024 (direct, workspace 0), 1 025 with a short last chunk (merge route), cover check
  non-finite       one NaN / one +inf in one channel: that channel NaN everywhere, the others inside their bounds.
                   With fmaxf / `a > best` in the forward kernels (read off the code, not yet run) the ReLU turns the
                   channel into zeros and these two tests fail."""
import functools

import numpy as np
import pytest
import torch

import bn_act_cases as BC
import torch_refs as R
from test_query_group_gpu import (BF16, GUARD, NAN_BITS, L, _fresh_guards, dev, guards_intact, nans,  # noqa: F401
                                  same_bits, within)

pytestmark = pytest.mark.gpu
EPS = BC.EPS
EINVAL, EUNSUPPORTED = -1, -3
F32 = torch.float32


def devt(t):
    """A device tensor moved in front of GUARD elements of finite slack (as dev() does for numpy arrays)."""
    buf = torch.full((t.numel() + GUARD,), 1, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape)


def filled(a):
    """An in/out array (running statistics) in a guarded buffer."""
    a = np.asarray(a, np.float32)
    t = nans(a.size)
    t.copy_(torch.from_numpy(a).reshape(-1).cuda())
    return t


_alive = []                        # device copies whose pointers went into a call: kept until the test ends


@pytest.fixture(autouse=True)
def _release():
    _alive.clear()
    yield
    _alive.clear()


def hold(a):
    """dev(a) (None stays None), alive until the end of the test: a tensor that exists only inside a call's argument list
    is freed, and its block handed to the next allocation, before the kernel runs."""
    t = None if a is None else dev(a)
    _alive.append(t)
    return t


opt = hold


def P_(L, t):
    return None if t is None else L.pptr(t, t.dtype)


def workspace(L, B, C, P):
    n = L.raw("mgar_bn_workspace_floats", B, C, P)
    assert n > 0
    return nans(n)


def twin(name, dtype):
    return name if dtype == F32 else name + "_bf16"


def bf16_pair(x):
    """x (numpy fp32) -> (bf16 device tensor, the same values widened to fp32), both with slack."""
    xb = dev(x).bfloat16()
    return devt(xb), devt(xb.float())


# ------------------------------------------------------------------------------------------------ statistics
@functools.lru_cache(maxsize=None)
def _stats_want(kind, name):
    k = BC.stats_case(name) if kind == "stats" else BC.grouped_case(name) if kind == "grouped" else BC.small_case(name)
    x = k["x"]
    per = kind == "grouped" or (kind == "small" and k["per_sample"])
    xs = x.reshape(1, -1, k["P"]) if per else x
    return (k,) + R.bn_train_stats_bounds(xs, EPS)


def _train_stats(L, x, B, C, P, grouped, momentum, running, k):
    dtype = x.dtype
    rows = B * C if grouped else C
    ws = workspace(L, 1, rows, P) if grouped else workspace(L, B, C, P)
    mean, invstd = nans(rows), nans(rows)
    rm, rv = (filled(k["running_mean"]), filled(k["running_var"])) if running else (None, None)
    nbt = dev(np.array([k["nbt"]], np.int64)) if running else None
    L.call(twin("mgar_bn_train_stats_grouped" if grouped else "mgar_bn_train_stats", dtype), L.pptr(x, dtype), B, C, P, EPS,
           momentum, L.fptr(ws), L.fptr(mean), L.fptr(invstd), P_(L, rm), P_(L, rv),
           nbt.data_ptr() if running else None, L.stream_of(x))
    return mean, invstd, rm, rv, nbt


def _check_stats(L, kind, name, momentum):
    grouped = kind == "grouped"
    k, mean, var, bmean, binv, bvar = _stats_want(kind, name)
    B, C, P = k["B"], k["C"], k["P"]
    x = dev(k["x"])
    got = _train_stats(L, x, B, C, P, grouped, momentum, True, k)
    bare = _train_stats(L, x, B, C, P, grouped, momentum, False, k)
    xb, xw = bf16_pair(k["x"])
    wide = _train_stats(L, xw, B, C, P, grouped, momentum, True, k)
    half = _train_stats(L, xb, B, C, P, grouped, momentum, True, k)
    guards_intact()
    within("%s mean" % name, got[0], mean, bmean)
    within("%s invstd" % name, got[1], (var + EPS) ** -0.5, binv)
    G = B if grouped else 1
    n = P if grouped else B * P
    rm, rv, brm, brv = R.bn_running_ref(mean.reshape(G, C), var.reshape(G, C), n, momentum, k["running_mean"],
                                        k["running_var"], bmean.reshape(G, C), bvar.reshape(G, C))
    within("%s running_mean" % name, got[2], rm, brm)
    within("%s running_var" % name, got[3], rv, brv)
    assert int(got[4][0]) == k["nbt"] + G
    same_bits("%s mean, running NULL" % name, bare[0], got[0])
    same_bits("%s invstd, running NULL" % name, bare[1], got[1])
    for i, what in enumerate(("mean", "invstd", "running_mean", "running_var")):
        same_bits("%s bf16 %s" % (name, what), half[i], wide[i])
    assert int(half[4][0]) == k["nbt"] + G
    return k, got


@pytest.mark.parametrize("name,momentum", [(n, m) for n in sorted(BC.STATS_CASES) for m in BC.MOMENTA
                                           if n != "chunk_32768" or m == 0.1])
def test_train_stats(L, name, momentum):
    """chunk_32768 runs at momentum 0.1 only: the case is about the chunking, and its 134 MB are uploaded per test."""
    k, got = _check_stats(L, "stats", name, momentum)
    if name == "n1":
        assert float(got[1][0]) == float(np.float32(1.0 / np.sqrt(EPS)))     # var = 0 exactly


@pytest.mark.parametrize("momentum", BC.MOMENTA)
@pytest.mark.parametrize("name", sorted(BC.GROUPED_CASES))
def test_train_stats_grouped_updates_in_sample_order(L, name, momentum):
    _check_stats(L, "grouped", name, momentum)


# ------------------------------------------------------------------------------------------------ apply
def _apply_all(L, k, relu, per_sample, dtype, x):
    """-> {route: y (B, C, P)} of act_fwd / act_fwd_grouped (contiguous) and act_fwd_into (y_bstride = C P + 8)."""
    B, C, P = k["B"], k["C"], k["P"]
    mean, invstd, gamma, beta = dev(k["mean"]), dev(k["invstd"]), opt(k["gamma"]), opt(k["beta"])
    stats = (L.fptr(mean), L.fptr(invstd), P_(L, gamma), P_(L, beta), relu)
    st = L.stream_of(x)
    y = nans(B * C * P, dtype)
    L.call(twin("mgar_bn_act_fwd_grouped" if per_sample else "mgar_bn_act_fwd", dtype), L.pptr(x, dtype), B, C, P, *stats,
           L.pptr(y, dtype), st)
    bs = C * P + BC.APPLY_PAD
    ys = nans(B * bs, dtype)
    L.call(twin("mgar_bn_act_fwd_into", dtype), L.pptr(x, dtype), B, C, P, *stats, per_sample, L.pptr(ys, dtype), bs, st)
    guards_intact()
    as_int, bits = NAN_BITS[dtype]
    assert (ys.view(B, bs)[:, C * P:].contiguous().view(as_int) == bits).all(), "the gap between two slices was written"
    return {"contiguous": y.view(B, C, P), "into": ys.view(B, bs)[:, :C * P].reshape(B, C, P)}


def _check_apply(L, k, relu, per_sample, tag):
    pre, want, bound = R.bn_apply_ref(k["x"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per_sample)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()               # the mask is the reference's
    for route, y in _apply_all(L, k, relu, per_sample, F32, dev(k["x"])).items():
        within("%s %s" % (tag, route), y, want, bound)
    xb, xw = bf16_pair(k["x"])
    y32, yb = _apply_all(L, k, relu, per_sample, F32, xw), _apply_all(L, k, relu, per_sample, BF16, xb)
    for route in y32:
        same_bits("%s %s bf16" % (tag, route), yb[route], y32[route].bfloat16())


@pytest.mark.parametrize("which", BC.APPLY_AFFINE)
@pytest.mark.parametrize("P", BC.APPLY_P)
def test_act_fwd_grouped_and_into(L, P, which):
    for per_sample in (0, 1):
        for relu in (1, 0):
            k = BC.apply_case(P, which, per_sample, relu=bool(relu))
            _check_apply(L, k, relu, per_sample, "P%d %s ps%d relu%d" % (P, which, per_sample, relu))


def test_act_fwd_at_mean_1e4(L):
    """(x - mean) * sc: the bound has no |mean| term, x * sc + (beta - mean * sc) would need one of 1e4 u |sc|."""
    for relu in (1, 0):
        k = BC.apply_case(4100, "both", 0, mean=1e4, relu=bool(relu))
        _check_apply(L, k, relu, 0, "mean1e4 relu%d" % relu)


# ------------------------------------------------------------------------------------------------ small fused
def _small(L, k, x, relu, full, strided):
    dtype = x.dtype
    B, C, P, per = k["B"], k["C"], k["P"], k["per_sample"]
    rows = B * C if per else C
    bs = C * P + BC.APPLY_PAD if strided else C * P
    y = nans(B * bs, dtype)
    mean, invstd = (nans(rows), nans(rows)) if full else (None, None)
    rm, rv = (filled(k["running_mean"]), filled(k["running_var"])) if full else (None, None)
    nbt = dev(np.array([k["nbt"]], np.int64)) if full else None
    ws = nans(rows) if full else None
    L.call(twin("mgar_bn_act_small", dtype), L.pptr(x, dtype), B, C, P, per, EPS, 0.1, L.fptr(hold(k["gamma"])),
           L.fptr(hold(k["beta"])), relu, P_(L, ws), P_(L, mean), P_(L, invstd), P_(L, rm), P_(L, rv),
           nbt.data_ptr() if full else None, L.pptr(y, dtype), bs if strided else -1, L.stream_of(x))
    guards_intact()
    as_int, bits = NAN_BITS[dtype]
    assert (y.view(B, bs)[:, C * P:].contiguous().view(as_int) == bits).all()
    return y.view(B, bs)[:, :C * P].reshape(B, C, P), mean, invstd, rm, rv, nbt


@pytest.mark.parametrize("name", sorted(BC.SMALL_CASES))
def test_act_small_against_float64_and_the_two_call_route(L, name):
    k, mean, var, bmean, binv, bvar = _stats_want("small", name)
    B, C, P, per = k["B"], k["C"], k["P"], k["per_sample"]
    G, n = (B, P) if per else (1, B * P)
    x = dev(k["x"])
    for relu in (1, 0):
        y, m_d, i_d, rm_d, rv_d, nbt = _small(L, k, x, relu, True, False)
        small_mean = m_d.double().cpu().numpy()
        within("%s mean" % name, m_d, mean, bmean)
        within("%s invstd" % name, i_d, (var + EPS) ** -0.5, binv)
        m32, i32 = m_d.cpu().numpy(), i_d.cpu().numpy()
        pre, want, bound = R.bn_apply_ref(k["x"], m32, i32, k["gamma"], k["beta"], relu, per)
        if relu:
            assert (np.abs(pre) > 2.0 * bound).all()
        within("%s y relu%d" % (name, relu), y, want, bound)
        rm, rv, brm, brv = R.bn_running_ref(mean.reshape(G, C), var.reshape(G, C), n, 0.1, k["running_mean"], k["running_var"],
                                            bmean.reshape(G, C), bvar.reshape(G, C))
        within("%s running_mean" % name, rm_d, rm, brm)
        within("%s running_var" % name, rv_d, rv, brv)
        assert int(nbt[0]) == k["nbt"] + G
        y2 = _small(L, k, x, relu, False, True)[0]
        same_bits("%s y, mean / invstd NULL, strided" % name, y2.contiguous(), y.contiguous())
    # the two-call route on the same input: the same bounds, and the two means agree within the two
    tm, ti, _, _, _ = _train_stats(L, x, B, C, P, bool(per), 0.1, True, k)
    within("%s two-call mean" % name, tm, mean, bmean)
    within("%s two-call invstd" % name, ti, (var + EPS) ** -0.5, binv)
    within("%s mean, one launch against two calls" % name, tm, small_mean, 2.0 * bmean)
    k2 = dict(k, mean=tm.cpu().numpy(), invstd=ti.cpu().numpy())
    pre, want, bound = R.bn_apply_ref(k["x"], k2["mean"], k2["invstd"], k["gamma"], k["beta"], 1, per)
    within("%s two-call y" % name, _apply_all(L, k2, 1, per, F32, x)["into"], want, bound)
    # bf16 twin
    xb, xw = bf16_pair(k["x"])
    w, h = _small(L, k, xw, 1, True, False), _small(L, k, xb, 1, True, False)
    same_bits("%s bf16 y" % name, h[0].contiguous(), w[0].bfloat16().contiguous())
    for i, what in ((1, "mean"), (2, "invstd"), (3, "running_mean"), (4, "running_var")):
        same_bits("%s bf16 %s" % (name, what), h[i], w[i])


@pytest.mark.parametrize("name", sorted(BC.SMALL_REJECTED))
def test_act_small_rejects_what_it_cannot_hold(L, name):
    B, C, P, per = BC.SMALL_REJECTED[name]
    x, y = dev(np.zeros((B, C, P), np.float32)), nans(B * C * P)
    for entry, dt in (("mgar_bn_act_small", F32), ("mgar_bn_act_small_bf16", BF16)):
        rc = L.raw(entry, x.data_ptr(), B, C, P, per, EPS, 0.1, None, None, 1, None, None, None, None, None, None, y.data_ptr(), -1,
                   L.stream_of(x))
        assert rc == EUNSUPPORTED
    guards_intact()
    assert torch.isnan(y).all()


# ------------------------------------------------------------------------------------------------ max-pool forward
def _maxpool(L, k, x, relu, with_xarg):
    dtype = x.dtype
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    out, xarg = nans(B * C * M, dtype), nans(B * C * M, dtype) if with_xarg else None
    arg = torch.full((B * C * M + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    L.call(twin("mgar_bn_act_maxpool_fwd", dtype), L.pptr(x, dtype), B, C, M, ns, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])),
           L.fptr(hold(k["gamma"])), L.fptr(hold(k["beta"])), relu, L.pptr(out, dtype), arg.data_ptr(), P_(L, xarg),
           L.stream_of(x))
    guards_intact()
    assert (arg[B * C * M:] == 0xA5).all(), "wrote behind arg"
    shape = (B, C, M)
    return out.view(shape), arg[:B * C * M].view(shape), None if xarg is None else xarg.view(shape)


def _check_maxpool(L, k, tag):
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    x = dev(k["x"])
    pre, _, bound = R.bn_apply_ref(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    pre, bound = pre.reshape(B, C, M, ns), bound.reshape(B, C, M, ns).max(-1)
    assert (np.abs(pre) > 2.0 * bound[..., None]).all()
    assert (pre[:, 3] < 0).all()                                 # the all-negative channel
    xb, xw = bf16_pair(k["x"])
    for relu in (1, 0):
        want, _ = R.bn_max_ref(pre, relu)
        out, arg, xarg = _maxpool(L, k, x, relu, True)
        within("%s relu%d max" % (tag, relu), out, want, bound)
        a = arg.cpu().numpy().astype(np.int64)
        assert a.max() < ns
        chosen = np.take_along_axis(pre, a[..., None], -1)[..., 0]
        assert (chosen >= pre.max(-1) - 2.0 * bound).all(), "%s: arg is not at a maximum" % tag
        assert (a[:, 2] == 0).all(), "gamma = 0: every slot ties, the first one wins"
        if k["ties"] is not None:
            first = np.broadcast_to(k["ties"][None, None, :], a.shape)
            assert (a[:, [0, 1, 3]] == first[:, [0, 1, 3]]).all(), "%s: not the first of two equal maxima" % tag
        if relu:
            assert (out[:, 3] == 0).all()
        same_bits("%s relu%d xarg" % (tag, relu), xarg, dev(np.take_along_axis(k["x"], a[..., None], -1)[..., 0]))
        out2, arg2, _ = _maxpool(L, k, x, relu, False)
        same_bits("%s relu%d max without xarg" % (tag, relu), out2, out)
        assert torch.equal(arg2, arg)
        ow, aw, xw_ = _maxpool(L, k, xw, relu, True)
        oh, ah, xh_ = _maxpool(L, k, xb, relu, True)
        same_bits("%s relu%d bf16 max" % (tag, relu), oh, ow.bfloat16())
        same_bits("%s relu%d bf16 xarg" % (tag, relu), xh_, xw_.bfloat16())
        assert torch.equal(ah, aw), "%s: bf16 arg differs" % tag


@pytest.mark.parametrize("name", sorted(BC.MAX_CASES))
def test_maxpool_fwd(L, name):
    _check_maxpool(L, BC.max_case(name), name)


@pytest.mark.parametrize("ns", BC.TIE_NS)
def test_maxpool_fwd_picks_the_first_of_equal_maxima(L, ns):
    _check_maxpool(L, BC.tie_case(ns), "ties ns%d" % ns)


def test_maxpool_fwd_rejects_nsample_256(L):
    x, out = dev(np.zeros((1, 1, 1, 256), np.float32)), nans(1)
    one = dev(np.ones(1, np.float32))
    arg = torch.zeros(1 + GUARD, dtype=torch.uint8, device="cuda")
    for entry in ("mgar_bn_act_maxpool_fwd", "mgar_bn_act_maxpool_fwd_bf16"):
        assert L.raw(entry, x.data_ptr(), 1, 1, 1, 256, one.data_ptr(), one.data_ptr(), None, None, 1, out.data_ptr(),
                     arg.data_ptr(), None, L.stream_of(x)) == EINVAL
    guards_intact()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ backward
def _lane_chain(B, C, P):
    nk = min(R.bn_chunk(B, C, P), B * P)
    return 4 * -(-nk // 1024) if P % 4 == 0 else -(-nk // 256)


def _bwd_want(k, relu, coef_given=False):
    pre, _, bound = R.bn_apply_ref(k["x"], k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()
    dz = k["dy"].astype(np.float64) * ((pre > 0) if relu else 1.0)
    r = R.bn_bwd_ref(dz, k["x"], k["mean"], k["invstd"], k["gamma"])
    return r, R.bn_bwd_bounds(r, _lane_chain(k["B"], k["C"], k["P"]), coef_given)


def _bwd(L, k, relu, entry, dy, x):
    dtype = x.dtype
    B, C, P = k["B"], k["C"], k["P"]
    ws, dgamma, dbeta, dx = workspace(L, B, C, P), nans(C), nans(C), nans(B * C * P, dtype)
    L.call(entry, L.pptr(dy, dtype), L.pptr(x, dtype), B, C, P, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])),
           P_(L, opt(k["gamma"])), P_(L, opt(k["beta"])), relu, L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.pptr(dx, dtype),
           L.stream_of(x))
    guards_intact()
    return dgamma, dbeta, dx


def _bwd_apply(L, k, relu, rowmajor, coef32):
    B, C, P = k["B"], k["C"], k["P"]
    x, dy, dx = dev(k["x"]), dev(k["dy"]), nans(B * C * P)
    L.call("mgar_bn_act_bwd_apply", L.fptr(dy), L.fptr(x), B, C, P, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])),
           P_(L, opt(k["gamma"])), P_(L, opt(k["beta"])), relu, L.fptr(hold(coef32)), rowmajor, L.fptr(dx), L.stream_of(x))
    guards_intact()
    return dx


def _check_bwd_apply(L, k, relu, rowmajor, tag):
    r, _ = _bwd_want(k, relu)
    coef32 = r["coef"].astype(np.float32)                      # float64 of the test, rounded: an input like mean / invstd
    B, C, P = k["B"], k["C"], k["P"]
    r2 = dict(r, coef=coef32.astype(np.float64))
    r2["dx"] = r["k"] * (r["dz"] - r2["coef"][:, 0].reshape(1, C, 1) - r["xh"] * r2["coef"][:, 1].reshape(1, C, 1))
    bdx = R.bn_bwd_bounds(r2, _lane_chain(B, C, P), coef_given=True)[3]
    got = _bwd_apply(L, k, relu, rowmajor, coef32)
    want = r2["dx"].transpose(0, 2, 1) if rowmajor else r2["dx"]
    within("%s bwd_apply" % tag, got.view(want.shape), want, bdx.transpose(0, 2, 1) if rowmajor else bdx)
    same_bits("%s bwd_apply second run" % tag, _bwd_apply(L, k, relu, rowmajor, coef32), got)


@pytest.mark.parametrize("which", ["both", "none"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("name", sorted(BC.BWD_CASES))
def test_act_bwd(L, name, relu, which):
    B, C, P = BC.BWD_CASES[name]
    k = BC.bwd_case(B, C, P, relu, which)
    tag = "%s relu%d %s" % (name, relu, which)
    r, (bbeta, bgamma, _, bdx) = _bwd_want(k, relu)
    x, dy = dev(k["x"]), dev(k["dy"])
    dgamma, dbeta, dx = _bwd(L, k, relu, "mgar_bn_act_bwd", dy, x)
    within("%s dgamma" % tag, dgamma, r["dgamma"], bgamma)
    within("%s dbeta" % tag, dbeta, r["dbeta"], bbeta)
    within("%s dx" % tag, dx.view(B, C, P), r["dx"], bdx)
    for a, b_, what in zip(_bwd(L, k, relu, "mgar_bn_act_bwd", dy, x), (dgamma, dbeta, dx), ("dgamma", "dbeta", "dx")):
        same_bits("%s %s second run" % (tag, what), a, b_)
    _check_bwd_apply(L, k, relu, 0, tag)
    xb, xw = bf16_pair(k["x"])
    db, dw = bf16_pair(k["dy"])
    w, h = _bwd(L, k, relu, "mgar_bn_act_bwd", dw, xw), _bwd(L, k, relu, "mgar_bn_act_bwd_bf16", db, xb)
    same_bits("%s bf16 dgamma" % tag, h[0], w[0])
    same_bits("%s bf16 dbeta" % tag, h[1], w[1])
    same_bits("%s bf16 dx" % tag, h[2], w[2].bfloat16())


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("P,C", BC.ROWMAJOR_CASES)
def test_act_bwd_rowmajor(L, P, C, relu):
    B = 2
    k = BC.bwd_case(B, C, P, relu, "both" if relu else "none", seed=5)
    tag = "rowmajor P%d C%d relu%d" % (P, C, relu)
    r, (bbeta, bgamma, _, bdx) = _bwd_want(k, relu)
    x, dy = dev(k["x"]), dev(k["dy"])
    dgamma, dbeta, dx_t = _bwd(L, k, relu, "mgar_bn_act_bwd_rowmajor", dy, x)
    within("%s dgamma" % tag, dgamma, r["dgamma"], bgamma)
    within("%s dbeta" % tag, dbeta, r["dbeta"], bbeta)
    within("%s dx_t" % tag, dx_t.view(B, P, C), r["dx"].transpose(0, 2, 1), bdx.transpose(0, 2, 1))
    for a, b_, what in zip(_bwd(L, k, relu, "mgar_bn_act_bwd_rowmajor", dy, x), (dgamma, dbeta, dx_t), ("dgamma", "dbeta", "dx_t")):
        same_bits("%s %s second run" % (tag, what), a, b_)
    _check_bwd_apply(L, k, relu, 1, tag)


def test_act_bwd_rowmajor_rejects_65_channels(L):
    B, C, P = 1, 65, 64
    z, one, out = dev(np.zeros((B, C, P), np.float32)), dev(np.ones(2 * C, np.float32)), nans(B * C * P)
    ws = workspace(L, B, C, P)
    p = z.data_ptr()
    assert L.raw("mgar_bn_act_bwd_rowmajor", p, p, B, C, P, one.data_ptr(), one.data_ptr(), None, None, 1, ws.data_ptr(), None, None,
                 out.data_ptr(), L.stream_of(z)) == EUNSUPPORTED
    assert L.raw("mgar_bn_act_bwd_apply", p, p, B, C, P, one.data_ptr(), one.data_ptr(), None, None, 1, one.data_ptr(), 1,
                 out.data_ptr(), L.stream_of(z)) == EUNSUPPORTED
    guards_intact()
    assert torch.isnan(out).all() and torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------ max-pool backward
def _dpool(k, layout):
    """(base tensor kept alive, pointer, (sb, sc, sm))"""
    B, C, M = k["B"], k["C"], k["M"]
    ct, c0 = BC.MAXBWD_CTOTAL, BC.MAXBWD_C0
    if layout == "contiguous":
        t = dev(k["dpool"])
        return t, t.data_ptr(), (C * M, M, 1)
    if layout == "channel_slice":
        t = dev(k["dpool_wide"])
        return t, t.data_ptr() + 4 * c0 * M, (ct * M, M, 1)
    t = dev(np.ascontiguousarray(k["dpool_wide"].transpose(0, 2, 1)))       # (B, M, C_total) rows
    return t, t.data_ptr() + 4 * c0, (M * ct, 1, ct)


def _maxbwd_want(k, relu):
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    x3 = k["x"].reshape(B, C, M * ns)
    pre, _, bound = R.bn_apply_ref(x3, k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    assert (np.abs(pre) > 2.0 * bound).all()
    pooled, arg = R.bn_max_ref(pre.reshape(B, C, M, ns), relu)
    d = np.where(pooled > 0, k["dpool"].astype(np.float64), 0.0) if relu else k["dpool"].astype(np.float64)   # +0, never -0
    dz = np.zeros((B, C, M, ns))
    np.put_along_axis(dz, arg[..., None], d[..., None], -1)
    r = R.bn_bwd_ref(dz.reshape(B, C, M * ns), x3, k["mean"], k["invstd"], k["gamma"])
    chain = -(-min(R.bn_chunk(B, C, M), B * M) // 256)
    return r, R.bn_bwd_bounds(r, chain), pooled.astype(np.float32), arg.astype(np.uint8), d.astype(np.float32)


def _fwd_state(k, pooled32, arg8, dtype=F32):
    x = dev(k["x"]).to(dtype)
    xarg = np.take_along_axis(k["x"], arg8.astype(np.int64)[..., None], -1)[..., 0]
    return devt(x), devt(dev(pooled32).to(dtype)), dev(arg8), devt(dev(xarg).to(dtype))


def _maxbwd(L, k, relu, layout, state, with_xarg, dtype=F32, dp=None):
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    x, pooled, arg, xarg = state
    keep, ptr, (sb, sc, sm) = dp if dp is not None else _dpool(k, layout)
    ws, dgamma, dbeta, dx = workspace(L, B, C, M * ns), nans(C), nans(C), nans(B * C * M * ns, dtype)
    head = (pooled.data_ptr(), arg.data_ptr(), x.data_ptr(), xarg.data_ptr() if with_xarg else None, B, C, M, ns,
            L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])), L.fptr(hold(k["gamma"])), relu, L.fptr(ws), L.fptr(dgamma),
            L.fptr(dbeta), dx.data_ptr(), L.stream_of(x))
    if layout == "contiguous":
        L.call(twin("mgar_bn_act_maxpool_bwd", dtype), ptr, *head)
    else:
        L.call("mgar_bn_act_maxpool_bwd_strided", ptr, sb, sc, sm, *head)
    guards_intact()
    return dgamma, dbeta, dx


def _maxbwd_reduce(L, k, relu, layout, state, with_xarg, explicit):
    B, C, M, ns = k["B"], k["C"], k["M"], k["ns"]
    x, pooled, arg, xarg = state
    keep, ptr, (sb, sc, sm) = _dpool(k, layout)
    if not explicit:
        sb, sc, sm = 0, -1, 0
    ws, dgamma, dbeta, coef, dmask = workspace(L, B, C, M * ns), nans(C), nans(C), nans(2 * C), nans(B * C * M)
    L.call("mgar_bn_act_maxpool_bwd_reduce", ptr, sb, sc, sm, pooled.data_ptr(), arg.data_ptr(), x.data_ptr(),
           xarg.data_ptr() if with_xarg else None, B, C, M, ns, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])), relu,
           L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(coef), L.fptr(dmask), L.stream_of(x))
    guards_intact()
    return dgamma, dbeta, coef, dmask


@pytest.mark.parametrize("layout", BC.DPOOL_LAYOUTS)
@pytest.mark.parametrize("ns", BC.MAXBWD_NS)
def test_maxpool_bwd_strided_and_reduce(L, ns, layout):
    k = BC.maxbwd_case(ns)
    B, C, M = k["B"], k["C"], k["M"]
    for relu in (1, 0):
        tag = "ns%d %s relu%d" % (ns, layout, relu)
        r, (bbeta, bgamma, bcoef, bdx), pooled32, arg8, d32 = _maxbwd_want(k, relu)
        state = _fwd_state(k, pooled32, arg8)
        dgamma, dbeta, dx = _maxbwd(L, k, relu, layout, state, True)
        within("%s dgamma" % tag, dgamma, r["dgamma"], bgamma)
        within("%s dbeta" % tag, dbeta, r["dbeta"], bbeta)
        within("%s dx" % tag, dx.view(B, C, M * ns), r["dx"], bdx)
        again, gathered = _maxbwd(L, k, relu, layout, state, True), _maxbwd(L, k, relu, layout, state, False)
        for i, what in enumerate(("dgamma", "dbeta", "dx")):
            same_bits("%s %s second run" % (tag, what), again[i], (dgamma, dbeta, dx)[i])
            same_bits("%s %s xarg NULL" % (tag, what), gathered[i], (dgamma, dbeta, dx)[i])
        for explicit in ((True, False) if layout == "contiguous" else (True,)):
            for with_xarg in (True, False):
                rg, rb, coef, dmask = _maxbwd_reduce(L, k, relu, layout, state, with_xarg, explicit)
                what = "%s reduce explicit%d xarg%d" % (tag, explicit, with_xarg)
                same_bits("%s dgamma" % what, rg, dgamma)
                same_bits("%s dbeta" % what, rb, dbeta)
                within("%s coef" % what, coef.view(C, 2), r["coef"], bcoef)
                same_bits("%s dmask" % what, dmask.view(B, C, M), dev(d32))
        if layout == "contiguous":
            sw = _fwd_state(k, pooled32, arg8, BF16)
            wide = tuple(devt(t.float()) if t.dtype == BF16 else t for t in sw)
            db, dw = bf16_pair(k["dpool"])
            shape = (C * M, M, 1)
            w = _maxbwd(L, k, relu, layout, wide, True, F32, (dw, dw.data_ptr(), shape))
            h = _maxbwd(L, k, relu, layout, sw, True, BF16, (db, db.data_ptr(), shape))
            same_bits("%s bf16 dgamma" % tag, h[0], w[0])
            same_bits("%s bf16 dbeta" % tag, h[1], w[1])
            same_bits("%s bf16 dx" % tag, h[2], w[2].bfloat16())


# ------------------------------------------------------------------------------------------------ statistics from partials
@pytest.mark.parametrize("momentum", BC.MOMENTA)
@pytest.mark.parametrize("name", sorted(BC.PARTIALS_CASES))
def test_stats_from_partials_direct_and_merge_route(L, name, momentum):
    k = BC.partials_case(name)
    C, nchunk = BC.PARTIALS_C, k["nchunk"]
    mean, var, bmean, binv, bvar = R.bn_from_partials_bounds(k["cnt"], k["partial"][:, :, 0], k["partial"][:, :, 1], EPS)
    nws = L.raw("mgar_bn_stats_from_partials_workspace_floats", nchunk, C)
    assert (nws > 0) == k["merge"]
    part = dev(k["partial"])
    outs = []
    for running in (True, False):
        ws = nans(nws) if nws else None
        m_d, i_d = nans(C), nans(C)
        rm, rv = (filled(k["running_mean"]), filled(k["running_var"])) if running else (None, None)
        nbt = dev(np.array([k["nbt"]], np.int64)) if running else None
        L.call("mgar_bn_stats_from_partials", L.fptr(part), nchunk, C, k["n"], k["chunk"], EPS, momentum, P_(L, ws), L.fptr(m_d),
               L.fptr(i_d), P_(L, rm), P_(L, rv), nbt.data_ptr() if running else None, L.stream_of(part))
        guards_intact()
        outs.append((m_d, i_d))
        within("%s mean" % name, m_d, mean, bmean)
        within("%s invstd" % name, i_d, (var + EPS) ** -0.5, binv)
        if running:
            wm, wv, brm, brv = R.bn_running_ref(mean, var, k["n"], momentum, k["running_mean"], k["running_var"], bmean, bvar)
            within("%s running_mean" % name, rm, wm, brm)
            within("%s running_var" % name, rv, wv, brv)
            assert int(nbt[0]) == k["nbt"] + 1
    same_bits("%s mean, running NULL" % name, outs[1][0], outs[0][0])
    # n that nchunk chunks do not cover, and n that fewer chunks cover already
    for n in (nchunk * k["chunk"] + 1, (nchunk - 1) * k["chunk"]):
        if n > 0:
            assert L.raw("mgar_bn_stats_from_partials", part.data_ptr(), nchunk, C, n, k["chunk"], EPS, momentum, None,
                         outs[0][0].data_ptr(), outs[0][1].data_ptr(), None, None, None, L.stream_of(part)) == EINVAL


# ------------------------------------------------------------------------------------------------ NaN and inf
def _all_nan(what, t):
    bad = int((~torch.isnan(t)).sum())
    assert bad == 0, "%s: %d of %d elements are not NaN" % (what, bad, t.numel())


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("P", [4100, 1367, 1028])
def test_a_non_finite_element_makes_its_channel_nan_through_relu(L, P, poison):
    """One NaN / +inf in channel 1 of (2, 3, P): torch's BatchNorm -> ReLU gives NaN everywhere in that channel (with +inf
    the mean is inf and the variance NaN).  Statistics + apply, and the one-launch kernel where it applies (P = 1 028)."""
    B, C = 2, 3
    rng = np.random.default_rng(P)
    clean = (0.7 + 2.0 * rng.standard_normal((B, C, P), dtype=np.float32)).astype(np.float32)
    gamma, beta = np.array([1.2, 0.8, -0.9], np.float32), np.array([0.3, -0.2, 0.4], np.float32)
    x = clean.copy()
    x[1, 1, 300] = poison
    k = dict(B=B, C=C, P=P, x=x, gamma=gamma, beta=beta, per_sample=0, running_mean=np.zeros(C, np.float32),
             running_var=np.ones(C, np.float32), nbt=0)
    ok = [0, 2]
    mean, var, bmean, binv, _ = R.bn_train_stats_bounds(clean, EPS)
    xd = dev(x)
    m_d, i_d, _, _, _ = _train_stats(L, xd, B, C, P, False, 0.1, True, k)
    routes = {"two-call": (m_d, i_d, _apply_all(L, dict(k, mean=m_d.cpu().numpy(), invstd=i_d.cpu().numpy()), 1, 0, F32, xd)["into"])}
    if P % 4 == 0 and B * P <= 16384:
        y, sm, si, _, _, _ = _small(L, k, xd, 1, True, False)
        routes["small"] = (sm, si, y)
    for route, (m, i, y) in routes.items():
        tag = "%s P%d %s" % (route, P, poison)
        assert not torch.isfinite(m[1]) and torch.isnan(i[1]), "%s: mean %s invstd %s" % (tag, m[1].item(), i[1].item())
        _all_nan("%s y of the poisoned channel" % tag, y[:, 1])
        within("%s mean of the clean channels" % tag, m[ok], mean[ok], bmean[ok])
        within("%s invstd of the clean channels" % tag, i[ok], ((var + EPS) ** -0.5)[ok], binv[ok])
        pre, want, bound = R.bn_apply_ref(clean, m.cpu().numpy(), i.cpu().numpy(), gamma, beta, 1)
        within("%s y of the clean channels" % tag, y[:, ok], want[:, ok], bound[:, ok])


@pytest.mark.parametrize("ns", [16, 5])
def test_a_nan_activation_makes_its_group_maximum_nan(L, ns):
    """Finite statistics, one NaN in x: torch.max gives NaN for that group (vector kernel, generic kernel), every other group
    stays inside its bound; a NaN mean makes every maximum of the channel NaN."""
    k = BC.max_case("ns16_m300") if ns == 16 else BC.max_case("ns5_m257")
    B, C, M = k["B"], k["C"], k["M"]
    x = k["x"].copy()
    hit = [(0, 0, 3, ns - 1), (0, 1, M - 1, 0), (0, 3, 7, 2)]
    for h in hit:
        x[h] = np.nan
    mean = k["mean"].copy()
    mean[2] = np.nan                                             # gamma = 0 there: (x - NaN) * 0 is NaN all the same
    kk = dict(k, x=x, mean=mean)
    pre, _, bound = R.bn_apply_ref(k["x"].reshape(B, C, M * ns), k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    pre, bound = pre.reshape(B, C, M, ns), bound.reshape(B, C, M, ns).max(-1)
    for relu in (1, 0):
        want, _ = R.bn_max_ref(pre, relu)
        out, arg, xarg = _maxpool(L, kk, dev(x), relu, True)
        expect_nan = np.zeros((B, C, M), bool)
        expect_nan[:, 2] = True
        for b, c, m, s in hit:
            expect_nan[b, c, m] = True
            assert int(arg[b, c, m]) == s, "arg of a NaN group is the NaN's slot, as torch.max"
        got_nan = torch.isnan(out).cpu().numpy()
        assert np.array_equal(got_nan, expect_nan), "relu%d: %d groups differ" % (relu, (got_nan != expect_nan).sum())
        fin = ~expect_nan
        within("ns%d relu%d the other groups" % (ns, relu), out.cpu().numpy()[fin], want[fin], bound[fin])


def test_every_entry_point_of_the_header_is_named_here():
    import re
    from multimodal_gar_amd import _lib
    src = open(__file__).read()
    skip = ("mgar_bn_cl_", "mgar_bn_rows_", "mgar_bn_act_fwd_to_cl")          # channels_last.hpp: their own tests
    names = [n for n in _lib._protos if n.startswith("mgar_bn_") and not n.startswith(skip)]
    assert len(names) >= 25
    for n in names:
        base = n[:-5] if n.endswith("_bf16") else n
        assert re.search(r'"%s"' % base, src), n
