"""Channels-last / row-major BatchNorm (csrc/channels_last.hpp): mgar_bn_cl_train_stats, mgar_bn_cl_act_fwd,
mgar_bn_act_fwd_to_cl, mgar_bn_rows_bwd and their bf16 twins against the float64 references of torch_refs.py on the hand-built
inputs of channels_last_cases.py.  tests/test_channels_last_cpu.py shows, with no kernel, that the references are torch's
BatchNorm chain, that the bounds are satisfiable and that they bite.  The bounds are rounding counts,
none is fitted to a kernel's output.  The channels-last pool (mgar_maxpool3d_same_fwd_cl) is in tests/test_maxpool3d_gpu.py.

Calls go through `_lib` with raw pointers; dev(), nans(), guards_intact(), within(), same_bits() are those of
tests/test_query_group_gpu.py, devt(), filled(), hold() those of tests/test_bn_act_gpu.py (imported, not copied): every
output and every workspace (sized by the library's own size query) starts as payload NaNs with a guard behind that must keep
its bits, and every comparison logs the share of its bound that it used.  The backward runs twice and must be bit-equal.

Which case covers which edge:
  statistics  C = 4 (256 row lanes), 24 (rpar 42, four idle threads), 516 (rpar 1, 127 idle), 1024 (no row lanes); one row
              (var 0 exactly), 7 rows under 64 lanes, a last chunk of one row, chunk 293 > 256 over 600 000 rows; per-sample
              S = 3 with far-apart samples (updates in sample order), S = 3 with chunks that cross samples, mean 1e4, an
              outlier in the pivot row; running_* / num_batches_tracked given and NULL, momentum 0.1 and 1.0
  apply       the same C, ldy = C and C + 8 (the gap keeps its bits), gamma / beta NULL in every combination, gamma < 0 and
              = 0, relu 0 / 1, per-sample S = 3 R = 5, total one past a multiple of 256
  to NDHWC    R in {1, 63, 64, 65} x C in {1, 3, 64, 65} around the 64 x 64 tile, S = 2, per-sample 0 / 1, ldy = C and C + 8
  backward    rows 1, 7, 257, 300, 600 000 (chunk 293) x C 4, 8, 24, 516, 1024, relu 0 / 1, gamma / beta NULL
  non-finite  one NaN in x: NaN there and nowhere else; a NaN mean under gamma = 0: the whole channel; statistics + apply
              with a NaN / +inf in x: that channel NaN everywhere.  With fmaxf in the apply kernels the ReLU returns 0."""
import functools

import numpy as np
import pytest
import torch

import channels_last_cases as CC
import torch_refs as R
from test_bn_act_gpu import F32, P_, _release, bf16_pair, devt, filled, hold, twin  # noqa: F401
from test_query_group_gpu import (BF16, GUARD, NAN_BITS, L, _fresh_guards, dev, guards_intact, nans,  # noqa: F401
                                  same_bits, within)

pytestmark = pytest.mark.gpu
EPS = CC.EPS
EINVAL = -1


# ------------------------------------------------------------------------------------------------ statistics
@functools.lru_cache(maxsize=None)
def _stats_want(name):
    k = CC.stats_case(name)
    return (k,) + R.bn_cl_train_stats_bounds(k["x"], k["per_sample"], EPS)


def _train_stats(L, x, S, Rr, C, per, momentum, running, k):
    dtype = x.dtype
    n = L.raw("mgar_bn_cl_workspace_floats", S, Rr, C, per)
    assert n > 0
    ws, rows = nans(n), (S * C if per else C)
    mean, invstd = nans(rows), nans(rows)
    rm, rv = (filled(k["running_mean"]), filled(k["running_var"])) if running else (None, None)
    nbt = dev(np.array([k["nbt"]], np.int64)) if running else None
    L.call(twin("mgar_bn_cl_train_stats", dtype), L.pptr(x, dtype), S, Rr, C, per, EPS, momentum, L.fptr(ws), L.fptr(mean),
           L.fptr(invstd), P_(L, rm), P_(L, rv), nbt.data_ptr() if running else None, L.stream_of(x))
    return mean, invstd, rm, rv, nbt


@pytest.mark.parametrize("momentum", CC.MOMENTA)
@pytest.mark.parametrize("name", sorted(CC.STATS_CASES))
def test_cl_train_stats(L, name, momentum):
    k, mean, var, bmean, binv, bvar = _stats_want(name)
    S, Rr, C, per = k["S"], k["R"], k["C"], k["per_sample"]
    x = dev(k["x"])
    got = _train_stats(L, x, S, Rr, C, per, momentum, True, k)
    bare = _train_stats(L, x, S, Rr, C, per, momentum, False, k)
    xb, xw = bf16_pair(k["x"])
    wide = _train_stats(L, xw, S, Rr, C, per, momentum, True, k)
    half = _train_stats(L, xb, S, Rr, C, per, momentum, True, k)
    guards_intact()
    within("%s mean" % name, got[0], mean, bmean)
    within("%s invstd" % name, got[1], (var + EPS) ** -0.5, binv)
    G, n = (S, Rr) if per else (1, S * Rr)
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
    if name == "one_row":
        assert (got[1] == float(np.float32(1.0 / np.sqrt(EPS)))).all()       # var = 0 exactly
        same_bits("one row: the mean is the row", got[0], x.view(-1))


# ------------------------------------------------------------------------------------------------ apply
def _gap_intact(y, rows, C, ldy, dtype):
    as_int, bits = NAN_BITS[dtype]
    if ldy > C:
        assert (y.view(rows, ldy)[:, C:].contiguous().view(as_int) == bits).all(), "the columns beside the slice were written"


def _apply(L, k, relu, per, x, ldy, entry="mgar_bn_cl_act_fwd"):
    """-> y (S, R, C): the first C columns of a (S * R, ldy) buffer."""
    dtype = x.dtype
    S, Rr, C = k["S"], k["R"], k["C"]
    rows = S * Rr
    y = nans(rows * ldy, dtype)
    sizes = (S, C, Rr) if entry == "mgar_bn_act_fwd_to_cl" else (S, Rr, C)
    L.call(twin(entry, dtype), L.pptr(x, dtype), *sizes, per, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])),
           P_(L, hold(k["gamma"])), P_(L, hold(k["beta"])), relu, L.pptr(y, dtype), ldy, L.stream_of(x))
    guards_intact()
    _gap_intact(y, rows, C, ldy, dtype)
    return y.view(rows, ldy)[:, :C].reshape(S, Rr, C)


def _check_apply(L, k, relu, per, tag, entry="mgar_bn_cl_act_fwd"):
    C = k["C"]
    pre, want, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], relu, per)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()               # the mask is the reference's
    src = k["xc"] if entry == "mgar_bn_act_fwd_to_cl" else k["x"]
    xb, xw = bf16_pair(src)
    for ldy in (C, C + CC.APPLY_PAD):
        y = _apply(L, k, relu, per, dev(src), ldy, entry)
        within("%s ldy%d" % (tag, ldy), y, CC.to_rows(want), CC.to_rows(bound))
        y32, yb = _apply(L, k, relu, per, xw, ldy, entry), _apply(L, k, relu, per, xb, ldy, entry)
        same_bits("%s ldy%d bf16" % (tag, ldy), yb.contiguous(), y32.bfloat16().contiguous())


@pytest.mark.parametrize("which", CC.APPLY_AFFINE)
@pytest.mark.parametrize("C", CC.APPLY_C)
def test_cl_act_fwd(L, C, which):
    for per in (0, 1):
        for relu in (1, 0):
            _check_apply(L, CC.apply_case(3, 5, C, which, per, bool(relu)), relu, per, "C%d %s ps%d relu%d" % (C, which, per, relu))


@pytest.mark.parametrize("which", CC.APPLY_AFFINE)
def test_cl_act_fwd_total_one_past_a_multiple_of_256(L, which):
    _check_apply(L, CC.apply_case(1, 257, 4, which, 0), 1, 0, "total257 %s" % which)


@pytest.mark.parametrize("C", CC.TO_CL_C)
@pytest.mark.parametrize("Rr", CC.TO_CL_R)
def test_act_fwd_to_cl(L, Rr, C):
    for per in (0, 1):
        for relu in (1, 0):
            k = CC.to_cl_case(Rr, C, per, bool(relu))
            _check_apply(L, k, relu, per, "to_cl R%d C%d ps%d relu%d" % (Rr, C, per, relu), "mgar_bn_act_fwd_to_cl")


# ------------------------------------------------------------------------------------------------ backward
def _rows_bwd(L, k, relu, with_grads=True):
    rows, C = k["rows"], k["C"]
    n = L.raw("mgar_bn_rows_bwd_workspace_floats", rows, C)
    assert n > 0
    x, dy = hold(k["x"]), hold(k["dy"])
    ws, dgamma, dbeta, dx = nans(n), nans(C), nans(C), nans(rows * C)
    L.call("mgar_bn_rows_bwd", L.fptr(dy), L.fptr(x), rows, C, L.fptr(hold(k["mean"])), L.fptr(hold(k["invstd"])),
           P_(L, hold(k["gamma"])), P_(L, hold(k["beta"])), relu, L.fptr(ws), L.fptr(dgamma) if with_grads else None,
           L.fptr(dbeta) if with_grads else None, L.fptr(dx), L.stream_of(x))
    guards_intact()
    return dgamma, dbeta, dx.view(rows, C)


@pytest.mark.parametrize("which", ["both", "none"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("name", sorted(CC.BWD_CASES))
def test_rows_bwd(L, name, relu, which):
    k = CC.bwd_case(name, relu, which)
    rows, C = k["rows"], k["C"]
    tag = "%s relu%d %s" % (name, relu, which)
    pre, _, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 0)
    if relu:
        assert (np.abs(pre) > 2.0 * bound).all()
    dz = k["dyc"].astype(np.float64) * ((pre > 0) if relu else 1.0)
    r = R.bn_bwd_ref(dz, k["xc"], k["mean"], k["invstd"], k["gamma"])
    bbeta, bgamma, _, bdx = R.bn_bwd_bounds(r, R.bn_rows_bwd_lane_chain(rows, C))
    dgamma, dbeta, dx = _rows_bwd(L, k, relu)
    within("%s dgamma" % tag, dgamma, r["dgamma"], bgamma)
    within("%s dbeta" % tag, dbeta, r["dbeta"], bbeta)
    within("%s dx" % tag, dx, r["dx"][0].T, bdx[0].T)
    for a, b_, what in zip(_rows_bwd(L, k, relu), (dgamma, dbeta, dx), ("dgamma", "dbeta", "dx")):
        same_bits("%s %s second run" % (tag, what), a, b_)
    same_bits("%s dx, dgamma / dbeta NULL" % tag, _rows_bwd(L, k, relu, False)[2], dx)


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_leave_the_outputs_untouched(L):
    x, y = dev(np.zeros((2, 8, 1028), np.float32)), nans(2 * 8 * 1028)
    one = dev(np.ones(65536, np.float32))
    st = L.stream_of(x)
    p, q, o = x.data_ptr(), y.data_ptr(), one.data_ptr()
    for sfx, esz in (("", 4), ("_bf16", 2)):
        for S, Rr, C in CC.CL_REJECTED_SHAPES.values():
            assert L.raw("mgar_bn_cl_train_stats" + sfx, p, S, Rr, C, 0, EPS, 0.1, q, q, q, None, None, None, st) == EINVAL
            assert L.raw("mgar_bn_cl_act_fwd" + sfx, p, S, Rr, C, 0, o, o, None, None, 1, q, C, st) == EINVAL
        S, Rr, C = CC.S_TIMES_C_TOO_LARGE
        assert L.raw("mgar_bn_cl_train_stats" + sfx, p, S, Rr, C, 1, EPS, 0.1, q, q, q, None, None, None, st) == EINVAL
        assert L.raw("mgar_bn_cl_act_fwd" + sfx, p, 2, 8, 8, 0, o, o, None, None, 1, q, 4, st) == EINVAL
        assert L.raw("mgar_bn_cl_act_fwd" + sfx, p, 2, 8, 8, 0, o, o, None, None, 1, q, 10, st) == EINVAL
        assert L.raw("mgar_bn_cl_act_fwd" + sfx, p, 2, 8, 8, 0, o, o, None, None, 1, q + esz, 8, st) == EINVAL
        assert L.raw("mgar_bn_cl_act_fwd" + sfx, None, 2, 8, 8, 0, o, o, None, None, 1, q, 8, st) == EINVAL
        assert L.raw("mgar_bn_act_fwd_to_cl" + sfx, p, 2, 8, 8, 0, o, o, None, None, 1, q, 7, st) == EINVAL
        assert L.raw("mgar_bn_cl_act_fwd" + sfx, None, 0, 8, 8, 0, None, None, None, None, 1, None, 8, st) == 0
        assert L.raw("mgar_bn_act_fwd_to_cl" + sfx, None, 2, 8, 0, 0, None, None, None, None, 1, None, 8, st) == 0
    assert L.raw("mgar_bn_rows_bwd", p, p, 8, 6, o, o, None, None, 1, q, None, None, q, st) == EINVAL
    assert L.raw("mgar_bn_rows_bwd", p, p, 8, 1028, o, o, None, None, 1, q, None, None, q, st) == EINVAL
    assert L.raw("mgar_bn_rows_bwd_workspace_floats", 8, 6) == -1
    assert L.raw("mgar_bn_rows_bwd", None, None, 0, 8, None, None, None, None, 1, None, None, None, None, st) == 0
    guards_intact()
    assert torch.isnan(y).all()


# ------------------------------------------------------------------------------------------------ NaN and inf
def _nan_set(what, got, want_nan):
    got_nan = torch.isnan(got.float()).cpu().numpy()
    assert np.array_equal(got_nan, want_nan), "%s: %d elements NaN, %d expected, %d differ" % (
        what, got_nan.sum(), want_nan.sum(), (got_nan != want_nan).sum())


@pytest.mark.parametrize("entry", ["mgar_bn_cl_act_fwd", "mgar_bn_act_fwd_to_cl"])
def test_a_nan_passes_the_relu_of_the_apply_kernels(L, entry):
    """One NaN in x: NaN at that element and nowhere else.  A NaN mean for a channel with gamma = 0: (x - NaN) * 0 is NaN all
    the same, the whole channel.  fp32 and bf16."""
    S, Rr, C = 2, 65, 8
    k = CC.apply_case(S, Rr, C, "both", 0)
    assert k["gamma"][2] == 0
    _, want, bound = R.bn_apply_ref(k["xc"], k["mean"], k["invstd"], k["gamma"], k["beta"], 1)
    want, bound = CC.to_rows(want), CC.to_rows(bound)
    for dtype in (F32, BF16):
        for site in ("x", "mean"):
            kk = dict(k, xc=k["xc"].copy(), mean=k["mean"].copy())
            expect = np.zeros((S, Rr, C), bool)
            if site == "x":
                kk["xc"][1, 5, 64] = np.nan
                expect[1, 64, 5] = True
            else:
                kk["mean"][2] = np.nan
                expect[:, :, 2] = True
            kk["x"] = CC.to_rows(kk["xc"])
            src = dev(kk["xc"] if entry == "mgar_bn_act_fwd_to_cl" else kk["x"]).to(dtype)
            y = _apply(L, kk, 1, 0, devt(src), C + CC.APPLY_PAD, entry)
            tag = "%s %s NaN in %s" % (entry, dtype, site)
            _nan_set(tag, y, expect)
            if dtype == F32:
                within("%s: the other elements" % tag, y.cpu().numpy()[~expect], want[~expect], bound[~expect])


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_row_makes_its_channel_nan_through_statistics_and_relu(L, poison):
    """The sparse trunk's training BatchNorm1d: one NaN / +inf in channel 5 of (300, 8) rows -> torch gives NaN everywhere in
    that channel (with +inf the mean is inf and the variance NaN); the other channels stay inside their bounds."""
    S, Rr, C = 1, 300, 8
    rng = np.random.default_rng(11)
    clean = (0.7 + 2.0 * rng.standard_normal((S, Rr, C), dtype=np.float32)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.5, 0.5, C).astype(np.float32)
    x = clean.copy()
    x[0, 270, 5] = poison                                         # in the ragged second chunk
    ok = [c for c in range(C) if c != 5]
    k = dict(S=S, R=Rr, C=C, running_mean=np.zeros(C, np.float32), running_var=np.ones(C, np.float32), nbt=0, gamma=gamma, beta=beta)
    mean, var, bmean, binv, _ = R.bn_cl_train_stats_bounds(clean, 0, EPS)
    xd = dev(x)
    m, i, _, _, _ = _train_stats(L, xd, S, Rr, C, 0, 0.1, True, k)
    y = _apply(L, dict(k, mean=m.cpu().numpy(), invstd=i.cpu().numpy()), 1, 0, xd, C)
    assert not torch.isfinite(m[5]) and torch.isnan(i[5]), "mean %s invstd %s" % (m[5].item(), i[5].item())
    expect = np.zeros((S, Rr, C), bool)
    expect[:, :, 5] = True
    _nan_set("y after %s" % poison, y, expect)
    within("mean of the clean channels", m[ok], mean[ok], bmean[ok])
    within("invstd of the clean channels", i[ok], ((var + EPS) ** -0.5)[ok], binv[ok])
    _, want, bound = R.bn_apply_ref(CC.to_bcp(clean)[:, ok], m.cpu().numpy()[ok], i.cpu().numpy()[ok], gamma[ok], beta[ok], 1)
    within("y of the clean channels", y.cpu().numpy()[:, :, ok], CC.to_rows(want), CC.to_rows(bound))


def test_every_entry_point_of_channels_last_and_maxpool3d_is_named_in_the_two_files():
    import os
    from multimodal_gar_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(__file__).read() + open(os.path.join(here, "test_maxpool3d_gpu.py")).read()
    names = [n for n in _lib._protos if n.startswith(("mgar_bn_cl_", "mgar_bn_rows_", "mgar_bn_act_fwd_to_cl", "mgar_maxpool3d_"))]
    assert len(names) >= 15
    for n in names:
        base = n[:-5] if n.endswith("_bf16") else n
        assert '"%s"' % base in src, n                            # the whole name, closing quote included
