"""A NaN must come out of the forward kernels as a NaN (csrc/bn_act.hip:41-45 states the rule: ReLU and running maxima propagate
NaN as torch.relu / torch.max do; fmaxf(NaN, 0) is 0 and NaN > best is false, so a diverged channel would come out as zeros
and training would go on with a finite loss).  Here: the BatchNorm + ReLU operand prologues of the shared-MLP convolution
(csrc/pointwise_fwd.hip, csrc/pointwise_dw.hip) and the training forward of Voxel-RoI pooling (csrc/voxel_roi_pool.hip).  The
channels-last BatchNorm kernels and the six pool entries have their non-finite tests next to their other op-level tests
(tests/test_channels_last_ops_gpu.py, tests/test_maxpool3d_gpu.py).

Each test plants one NaN in an otherwise ordinary small case and asserts that the set of NaN outputs is the float64
reference's set, and that every other output stays inside the tolerance of the entry's own parity test."""
import numpy as np
import pytest
import torch

import torch_refs as R
from test_bn_act_gpu import _release, devt  # noqa: F401
from test_query_group_gpu import BF16, GUARD, L, _fresh_guards, dev, guards_intact, nans, within  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _nan_set(what, got, want_nan):
    got_nan = torch.isnan(got.float()).cpu().numpy()
    assert np.array_equal(got_nan, want_nan), "%s: %d outputs NaN, %d expected, %d differ" % (
        what, got_nan.sum(), want_nan.sum(), (got_nan != want_nan).sum())


def _close(what, got, want, rtol, atol):
    """test_fusion_ops_gpu.close on the finite part: max err <= atol + rtol * max |want|."""
    err, scale = np.abs(got - want).max(), np.abs(want).max() + 1e-12
    assert err <= atol + rtol * scale, "%s: max err %g vs scale %g" % (what, err, scale)


# ------------------------------------------------------------------------------------------------ shared-MLP convolution
def _pw_case(B, Cin, Cout, P, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    return dict(x=f(B, Cin, P), w=f(Cout, Cin), dy=f(B, Cout, P), mean=f(Cin), invstd=(rng.uniform(0.5, 1.5, Cin) ** -0.5).astype(np.float32),
                gamma=f(Cin), beta=f(Cin))


def _pw_act64(k, x):
    v = lambda a: k[a].astype(np.float64)[None, :, None]   # noqa: E731
    return np.maximum((x.astype(np.float64) - v("mean")) * v("invstd") * v("gamma") + v("beta"), 0.0)


@pytest.mark.parametrize("entry", ["mgar_pointwise_conv_fwd", "mgar_pointwise_conv_fwd_bf16", "mgar_pointwise_conv_fwd_stats"])
def test_a_nan_activation_reaches_its_output_column_of_the_pointwise_convolution(L, entry):
    """x[1, 5, 300] = NaN behind the BN + ReLU prologue: y[1, :, 300] is NaN for every output channel, every other column is
    finite and within test_pointwise_conv_fwd_matches_fp64's tolerance (bf16: the fp32 entry on the widened values, rounded)."""
    B, Cin, Cout, P = 2, 12, 24, 1792
    k = _pw_case(B, Cin, Cout, P, 7)
    k["x"][1, 5, 300] = np.nan
    bf = entry.endswith("_bf16")
    x = dev(k["x"])
    if bf:
        x = devt(x.bfloat16())
    w, mean, invstd, gamma, beta = (dev(k[a]) for a in ("w", "mean", "invstd", "gamma", "beta"))
    y = nans(B * Cout * P, x.dtype)
    head = (L.pptr(x, x.dtype), B, Cin, P, L.fptr(w), Cin, 1, Cout, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta), 1,
            L.pptr(y, x.dtype))
    stats = None
    if entry.endswith("_stats"):
        # out_stats (Cout, B * P / 128, 2), chunk = 128: the size include/mgar_ops.h documents at the entry (it has no size query)
        stats = nans(Cout * (B * P // 128) * 2)
        L.call(entry, *head, L.fptr(stats), L.stream_of(x))
    else:
        L.call(entry, *head, L.stream_of(x))
    guards_intact()
    y = y.view(B, Cout, P)
    expect = np.zeros((B, Cout, P), bool)
    expect[1, :, 300] = True
    _nan_set(entry, y, expect)
    xv = x.float().cpu().numpy()
    clean = xv.copy()
    clean[1, 5, 300] = 0.0
    want = np.einsum("oi,bip->bop", k["w"].astype(np.float64), _pw_act64(k, clean))
    got = y.float().cpu().numpy().astype(np.float64)
    if bf:
        y32 = nans(B * Cout * P)
        xw = devt(x.float())
        L.call("mgar_pointwise_conv_fwd", L.fptr(xw), *head[1:-1], L.fptr(y32), L.stream_of(x))
        guards_intact()
        rounded = y32.view(B, Cout, P).bfloat16()
        assert np.array_equal(rounded.view(torch.int16).cpu().numpy()[~expect], y.view(torch.int16).cpu().numpy()[~expect])
        _close(entry, got[~expect], want[~expect], 2.0 ** -8, 1e-4)
    else:
        _close(entry, got[~expect], want[~expect], 2e-5, 1e-4)
    if stats is not None:            # the 128-column chunk that holds the NaN column, in every channel; no other chunk
        chunk_nan = torch.isnan(stats.view(Cout, B * P // 128, 2)[:, :, 0]).cpu().numpy()
        want_nan = np.zeros_like(chunk_nan)
        want_nan[:, (1 * P + 300) // 128] = True
        assert np.array_equal(chunk_nan, want_nan)


@pytest.mark.parametrize("B,Cin,Cout,P", [(1, 12, 24, 1776), (3, 64, 16, 1001)], ids=["vector_staging", "scalar_staging"])
def test_a_nan_activation_reaches_its_column_of_the_weight_gradient(L, B, Cin, Cout, P):
    """mgar_pointwise_conv_dw_act, P % 4 == 0 and P % 4 != 0: dW[:, 5] is NaN, every other column finite and within
    test_pointwise_conv_dw_act_matches_fp64's tolerance."""
    k = _pw_case(B, Cin, Cout, P, 9)
    clean = k["x"].copy()
    k["x"][B - 1, 5, P - 3] = np.nan
    x, dy, mean, invstd, gamma, beta = (dev(k[a]) for a in ("x", "dy", "mean", "invstd", "gamma", "beta"))
    ws = nans(L.raw("mgar_pointwise_dw_workspace_floats", B, Cin, Cout, P))
    dw = nans(Cout * Cin)
    L.call("mgar_pointwise_conv_dw_act", L.fptr(x), L.fptr(dy), B, Cin, Cout, P, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
           L.fptr(beta), 1, L.fptr(ws), L.fptr(dw), L.stream_of(x))
    guards_intact()
    expect = np.zeros((Cout, Cin), bool)
    expect[:, 5] = True
    _nan_set("dw_act P%d" % P, dw.view(Cout, Cin), expect)
    want = np.einsum("bop,bip->oi", k["dy"].astype(np.float64), _pw_act64(k, clean))
    _close("dw_act P%d" % P, dw.view(Cout, Cin).cpu().numpy().astype(np.float64)[~expect], want[~expect], 2e-5, 1e-3)


# ------------------------------------------------------------------------------------------------ Voxel-RoI pooling, training
def _vrp_case():
    """70 queries (two workgroups of 64) x 5 neighbours over 40 voxel rows, 8 channels.  Row 7 holds one NaN (channel 3), row 9 is
    NaN in every channel; query 2 names row 9 only (an all-NaN neighbourhood), queries 66 and 68 are empty (idx[m, 0] = -1 and
    arbitrary values behind)."""
    rng = np.random.default_rng(21)
    N, M, ns, C = 40, 70, 5, 8
    idx = rng.integers(10, N, (M, ns)).astype(np.int32)             # rows 0..9 only where the test puts them
    idx[5, 3], idx[5, 4] = 7, 7                                     # first NaN slot 3
    idx[64, 0] = 7                                                  # first slot, second workgroup
    idx[30, 1], idx[30, 2] = 9, 7                                   # an all-NaN row before the one-NaN row
    idx[2, :] = 9
    idx[66, 0], idx[68, 0] = -1, -1
    feats = rng.standard_normal((N, C)).astype(np.float32)
    clean = feats.copy()
    feats[7, 3] = np.nan
    feats[9, :] = np.nan
    f = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    return dict(N=N, M=M, ns=ns, C=C, idx=idx, feats=feats, clean=clean, xyz=f(N, 3), new_xyz=f(M, 3), w_pos=f(C, 3), mean=0.3 * f(C),
                invstd=rng.uniform(0.5, 2.0, C).astype(np.float32), gamma=f(C), beta=f(C))


def _vrp_ref(k, feats):
    """float64 pre-activations (M, C, ns) from the fp32 operands, and the rounding-count bound: at most 9 roundings on any term
    of f + ((w . r - mean) * (invstd * gamma) + beta) -- r, the product, two additions, - mean, invstd * gamma, the product
    with it, + beta, + f."""
    d = {a: k[a].astype(np.float64) for a in ("xyz", "new_xyz", "w_pos", "mean", "invstd", "gamma", "beta")}
    empty = k["idx"][:, 0] < 0
    rows = np.where(empty[:, None], 0, k["idx"])
    r = (d["xyz"][rows] - d["new_xyz"][:, None]) * ~empty[:, None, None]                       # (M, ns, 3)
    sc = d["invstd"] * d["gamma"]
    p = np.einsum("ck,msk->mcs", d["w_pos"], r)
    pabs = np.einsum("ck,msk->mcs", np.abs(d["w_pos"]), np.abs(r))
    f = feats.astype(np.float64)[rows].transpose(0, 2, 1) * ~empty[:, None, None]
    pre = f + ((p - d["mean"][None, :, None]) * sc[None, :, None] + d["beta"][None, :, None])
    mag = np.abs(np.nan_to_num(f)) + (pabs + np.abs(d["mean"])[None, :, None]) * np.abs(sc)[None, :, None] + np.abs(d["beta"])[None, :, None]
    return pre, R.gamma_u(9) * mag + R.TINY32


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_voxel_roi_pool_forward_pools_a_nan_row_to_nan_with_its_slot(L, dtype):
    k = _vrp_case()
    M, ns, C = k["M"], k["ns"], k["C"]
    feats = devt(dev(k["feats"]).to(dtype))
    fv = feats.float().cpu().numpy()
    pre, bound = _vrp_ref(k, fv)
    want = np.maximum(pre.max(-1), 0.0)                               # np.max and np.maximum propagate NaN
    want_arg = np.argmax(pre, -1)                                     # np.argmax: the first NaN, else the first maximum
    empty = k["idx"][:, 0] < 0
    expect = np.isnan(want)
    assert expect[2].all() and expect[30].all() and expect[5, 3] and expect[64, 3] and expect[5].sum() == 1 and not expect[empty].any()
    assert want_arg[5, 3] == 3 and want_arg[64, 3] == 0 and want_arg[30, 3] == 1 and (want_arg[2] == 0).all()
    xyz, new_xyz, idx, w_pos, mean, invstd, gamma, beta = (dev(k[a]) for a in ("xyz", "new_xyz", "idx", "w_pos", "mean", "invstd", "gamma", "beta"))
    pooled = nans(C * M, dtype)
    arg = torch.full((C * M + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    L.call("mgar_voxel_roi_pool_fwd" if dtype == F32 else "mgar_voxel_roi_pool_fwd_bf16", M, ns, C, L.fptr(xyz), L.fptr(new_xyz),
           L.pptr(feats, dtype), C, L.iptr(idx), L.fptr(w_pos), L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
           L.pptr(pooled, dtype), arg.data_ptr(), L.stream_of(xyz))
    guards_intact()
    assert (arg[C * M:] == 0xA5).all()
    got = pooled.view(C, M).t()
    got_arg = arg[:C * M].view(C, M).t().cpu().numpy().astype(np.int64)
    _nan_set("pooled", got, expect)
    assert np.array_equal(got_arg[expect], want_arg[expect]), "arg of a NaN maximum is the first NaN's slot, as torch.max"
    fin = ~expect
    b = bound.max(-1)
    g = got.float().cpu().numpy().astype(np.float64)
    if dtype == BF16:
        b = b + 2.0 ** -8 * (np.abs(np.nan_to_num(want)) + b)          # one rounding to bf16: 8 significant bits, u = 2^-8
    within("pooled, the finite entries (%s)" % dtype, g[fin], want[fin], b[fin])
    chosen = np.take_along_axis(pre, got_arg[..., None], -1)[..., 0]
    assert (chosen[fin] >= pre.max(-1)[fin] - 2.0 * bound.max(-1)[fin]).all(), "arg is not at a maximum"
    # empty neighbourhoods: relu(BN(0)) in every channel and slot 0, whatever the NaN rows hold
    bn0 = np.maximum((0.0 - k["mean"].astype(np.float64)) * (k["invstd"].astype(np.float64) * k["gamma"]) + k["beta"], 0.0)
    within("empty neighbourhoods", g[empty], np.broadcast_to(bn0, (int(empty.sum()), C)), b[empty])
    assert (got_arg[empty] == 0).all()
