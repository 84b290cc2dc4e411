"""Query-and-group (csrc/query_group.hip) -- what can be pinned without a GPU.

The device test (tests/test_query_group_gpu.py) compares the kernels with the float64 references of torch_refs.py on the
inputs of query_group_cases.py, inside bounds counted from roundings.  Here, with no kernel involved:

* the plain references ARE the reference's op chain: rounded to fp32 they reproduce, bit for bit, the C oracle's
  group_points, subtract-the-centre, (stack: zero the empty balls), concatenate;
* "project, then group" is algebra: the proj reference on zf = W_f . feat with wx equals W . [rel; feat], W = [wx | W_f],
  to 1e-12 in float64;
* the tile statistics merged with Chan's formula equal the direct float64 mean / biased variance to 1e-12;
* every bound the device test asserts is satisfiable on every case: the float64 reference rounded to fp32 stays inside it;
* the bounds bite: the kernel's summation order in numpy fp32 stays inside the statistics bounds while a sum-of-squares
  M2 leaves them in every cell of the shifted case, and a dropped wx term leaves the proj bound."""
import numpy as np
import pytest
import torch

import query_group_cases as QC
import torch_refs as R


def _f32(t):
    return torch.as_tensor(t).detach().double().float()


def _rel_err(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)


# ------------------------------------------------------------------------------------------------ references vs the oracle
@pytest.mark.parametrize("name", sorted(QC.BATCH_FWD_CASES))
def test_batch_reference_is_the_oracles_op_chain_bit_for_bit(oracle, name):
    k = QC.batch_fwd_case(name)
    rel, y = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"])
    near = oracle.group_points_batch(np.ascontiguousarray(k["xyz"].transpose(0, 2, 1)), k["idx"])
    chain = np.concatenate([near - k["new_xyz"].transpose(0, 2, 1)[:, :, :, None], oracle.group_points_batch(k["feats"], k["idx"])], 1)
    assert torch.equal(_f32(torch.cat([rel, y], 1)), torch.from_numpy(chain))


@pytest.mark.parametrize("C", QC.STACK_C)
@pytest.mark.parametrize("layout", sorted(QC.STACK_NEW_CNT))
def test_stack_reference_is_the_oracles_op_chain_bit_for_bit(oracle, layout, C):
    k = QC.stack_case(layout, C)
    rel, y = R.query_group_stack_ref(k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"], k["feats"], k["idx"])
    fixed = k["idx"].copy()
    fixed[k["empty"]] = 0                                    # pointnet2_stack/pointnet2_utils.py: idx[empty_ball_mask] = 0
    near = oracle.group_points_stack(k["xyz"], k["xyz_cnt"], fixed, k["new_cnt"]) - k["new_xyz"][:, :, None]
    feat = oracle.group_points_stack(k["feats"], k["xyz_cnt"], fixed, k["new_cnt"]) if C else np.zeros((k["M"], 0, k["ns"]), np.float32)
    near[k["empty"]] = 0
    feat[k["empty"]] = 0
    chain = np.concatenate([near, feat], 1).transpose(1, 0, 2).reshape(3 + C, -1)
    assert torch.equal(_f32(torch.cat([rel, y], 0)), torch.from_numpy(np.ascontiguousarray(chain)))
    assert k["empty"].sum() >= k["M"] // 7 and (k["idx"][k["empty"], 1:] != 0).all()


def test_stack_cases_are_what_they_claim():
    k = QC.stack_case("ragged", 32)
    rows = R.stack_source_rows(k["xyz_cnt"], k["new_cnt"], k["idx"])
    sample = np.repeat(np.arange(k["B"]), k["new_cnt"])
    assert sorted(set(sample[:8])) == [0, 2, 3]                                   # the first tile: three samples
    assert (k["M"] * k["ns"]) % 128 != 0
    start = np.concatenate([[0], np.cumsum(k["xyz_cnt"])[:-1]])
    assert (rows == start[3]).any() and (rows == start[3] + k["xyz_cnt"][3] - 1).any()
    assert k["empty"][sample == 2].all() and k["empty"][5] and k["empty"][154]    # no-point sample; first / last of sample 3
    t = QC.stack_case("tiles", 32)
    assert (t["M"] * t["ns"]) % 128 == 0
    assert t["empty"][QC.STACK_EMPTY_TILE * 8:(QC.STACK_EMPTY_TILE + 1) * 8].all()


# ------------------------------------------------------------------------------------------------ the identity of the route
@pytest.mark.parametrize("name", ["c9_cols255_b1", "c17_cols257_b3"])
def test_proj_batch_reference_is_the_first_layer_on_the_grouped_tensor(name):
    k = QC.batch_fwd_case(name)
    gen = torch.Generator().manual_seed(3)
    cin = 5
    feat = torch.randn(k["b"], cin, k["n"], dtype=torch.float64, generator=gen)
    w_f = torch.randn(k["c"], cin, dtype=torch.float64, generator=gen)
    wx = torch.from_numpy(k["wx"]).double()
    rel, grouped = R.query_group_batch_ref(k["xyz"], k["new_xyz"], feat, k["idx"])
    want = torch.einsum("ck,bkms->bcms", torch.cat([wx, w_f], 1), torch.cat([rel, grouped], 1))
    _, got = R.query_group_batch_ref(k["xyz"], k["new_xyz"], torch.einsum("ck,bkn->bcn", w_f, feat), k["idx"], wx)
    assert _rel_err(got, want) <= 1e-12


@pytest.mark.parametrize("C", [1, 33])
def test_proj_stack_reference_is_the_first_layer_on_the_grouped_tensor(C):
    k = QC.stack_case("ragged", C)
    gen = torch.Generator().manual_seed(4)
    cin = 6
    feat = torch.randn(k["N"], cin, dtype=torch.float64, generator=gen)
    w_f = torch.randn(C, cin, dtype=torch.float64, generator=gen)
    wx = torch.from_numpy(k["wx"]).double()
    args = (k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"])
    rel, grouped = R.query_group_stack_ref(*args, feat, k["idx"])
    want = torch.cat([wx, w_f], 1) @ torch.cat([rel, grouped], 0)
    _, got = R.query_group_stack_ref(*args, feat @ w_f.t(), k["idx"], wx)
    assert _rel_err(got, want) <= 1e-12


def test_stack_reference_ignores_garbage_and_passes_nothing_backward_through_empty_balls():
    k = QC.stack_case("ragged", 7)
    args = (k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"])
    zf = torch.from_numpy(k["feats"]).double().requires_grad_(True)
    wx = torch.from_numpy(k["wx"]).double().requires_grad_(True)
    rel, y = R.query_group_stack_ref(*args, zf, k["idx"], wx)
    cols = np.repeat(k["empty"], k["ns"])
    assert (rel[:, cols] == 0).all() and (y[:, cols] == 0).all()
    other = k["idx"].copy()
    other[k["empty"], 1:] = 1
    rel2, y2 = R.query_group_stack_ref(*args, zf, other, wx)
    assert torch.equal(rel, rel2) and torch.equal(y, y2)
    g = torch.from_numpy(k["g"][3:]).double()
    (y * g).sum().backward()
    rows = R.stack_source_rows(k["xyz_cnt"], k["new_cnt"], k["idx"])
    want, cnt, _ = R.qg_scatter_stack_ref(k["g"][3:], rows, k["N"])
    assert _rel_err(zf.grad, torch.from_numpy(want)) <= 1e-12
    assert (zf.grad[torch.from_numpy(cnt[:, 0] == 0)] == 0).all()
    live = torch.from_numpy(~cols)
    assert _rel_err(wx.grad, g[:, live] @ rel[:, live].t().detach()) <= 1e-12


# ------------------------------------------------------------------------------------------------ tile statistics
@pytest.mark.parametrize("shift,scale", [(0.0, 1.0), (100.0, 0.1)])
def test_tile_stats_merged_with_chans_formula_equal_the_direct_statistics(shift, scale):
    gen = torch.Generator().manual_seed(5)
    y = shift + scale * torch.randn(9, 20 * 128, dtype=torch.float64, generator=gen)
    y[:, 5 * 128:6 * 128] = 0
    tile_mean, tile_m2, mean, var = R.qg_tile_stats_ref(y)
    assert (tile_mean[:, 5] == 0).all() and (tile_m2[:, 5] == 0).all()
    assert _rel_err(mean, y.mean(1)) <= 1e-12
    assert _rel_err(var, y.var(1, unbiased=False)) <= 1e-12


# ------------------------------------------------------------------------------------------------ the bounds are satisfiable
@pytest.mark.parametrize("name", sorted(QC.BATCH_FWD_CASES))
def test_rounded_reference_is_inside_the_proj_batch_forward_bound(name):
    k = QC.batch_fwd_case(name)
    rel, y = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"], k["wx"])
    _, gathered = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"])
    bound = R.qg_proj_fwd_bound(gathered, k["wx"], rel)
    assert ((_f32(y).double() - y).abs() <= bound).all()


@pytest.mark.parametrize("C", QC.STACK_C)
@pytest.mark.parametrize("layout", sorted(QC.STACK_NEW_CNT))
def test_rounded_reference_is_inside_the_proj_stack_forward_bound(layout, C):
    k = QC.stack_case(layout, C)
    args = (k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"])
    rel, y = R.query_group_stack_ref(*args, k["feats"], k["idx"], k["wx"])
    _, gathered = R.query_group_stack_ref(*args, k["feats"], k["idx"])
    bound = R.qg_proj_fwd_bound(gathered, k["wx"], rel)
    assert ((_f32(y).double() - y).abs() <= bound).all()
    assert (bound[:, np.repeat(k["empty"], k["ns"])] == R.TINY32).all()


@pytest.mark.parametrize("cols", sorted(QC.BWD_COLS))
@pytest.mark.parametrize("n", QC.BWD_N)
def test_rounded_reference_is_inside_the_batch_backward_bounds(n, cols):
    k = QC.batch_bwd_case(n, cols)
    g = k["g"][:, 3:]
    want, cnt, sabs = R.qg_scatter_batch_ref(g, k["idx"], n)
    assert cnt.max() > 8 and (cnt == 0).any()
    assert {0, n - 1} <= set(k["idx"].reshape(-1).tolist())
    err = np.abs(want.astype(np.float32).astype(np.float64) - want)
    row_max = np.abs(g.astype(np.float64)).max(axis=2, keepdims=True)
    assert (err <= R.qg_fixed_point_scatter_bound(want, cnt, row_max, cols)).all()
    atomic = R.qg_atomic_scatter_bound(want, cnt, sabs)
    assert (err <= atomic).all() and (atomic[np.broadcast_to(cnt == 0, atomic.shape)] == 0).all()


@pytest.mark.parametrize("C", [c for c in QC.STACK_C if c])
@pytest.mark.parametrize("layout", sorted(QC.STACK_NEW_CNT))
def test_rounded_reference_is_inside_the_stack_backward_bound(layout, C):
    k = QC.stack_case(layout, C)
    rows = R.stack_source_rows(k["xyz_cnt"], k["new_cnt"], k["idx"])
    want, cnt, sabs = R.qg_scatter_stack_ref(k["g"][3:], rows, k["N"])
    assert cnt.max() > 8 and (cnt == 0).any()
    err = np.abs(want.astype(np.float32).astype(np.float64) - want)
    assert (err <= R.qg_atomic_scatter_bound(want, cnt, sabs)).all()


@pytest.mark.parametrize("C", [c for c in QC.STACK_C if c])
@pytest.mark.parametrize("shift,scale", [(0.0, 1.0), (100.0, 0.1)])
def test_rounded_reference_is_inside_the_tile_statistics_bounds(shift, scale, C):
    k = QC.stack_case("tiles", C, shift, scale, dense=bool(shift))
    _, y = R.query_group_stack_ref(k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"], k["feats"], k["idx"], k["wx"])
    y = _f32(y).double()                                     # the statistics are those of the fp32 tensor the kernel wrote
    tile_mean, tile_m2, mean, var = R.qg_tile_stats_ref(y)
    dmean, dm2 = R.qg_tile_stats_bounds(y)
    assert ((_f32(tile_mean).double() - tile_mean).abs() <= dmean).all()
    assert ((_f32(tile_m2).double() - tile_m2).abs() <= dm2).all()
    if not shift:
        assert (dmean[:, QC.STACK_EMPTY_TILE] == 0).all() and (dm2[:, QC.STACK_EMPTY_TILE] == 0).all()
    eps = 1e-5
    bmean, binv = R.qg_final_stats_bounds(y, eps)
    invstd = (var + eps) ** -0.5
    assert ((_f32(mean).double() - mean).abs() <= bmean).all()
    assert ((_f32(invstd).double() - invstd).abs() <= binv).all()
    # what the bounds are for: a sum / sum-of-squares M2 in fp32 errs by about u * sum v^2, far outside them when |mean| >> std
    if shift:
        assert (mean.abs() > 50.0 * var.sqrt()).all()
        assert (R.U32 * (y ** 2).view(y.shape[0], -1, 128).sum(2) > 100.0 * dm2).all()
        # ... and in the finalised variance by about u * mean^2 = 6e-4 against var = 1.3e-2: 2 % of invstd, bound 1e-3
        assert (binv / invstd).max().item() < 1e-3 < 0.1 * (0.5 * R.U32 * mean ** 2 / var).min().item()


# ------------------------------------------------------------------------------------------------ the bounds bite
def _tile_stats_fp32(y, two_pass):
    """qg_stack_fwd_kernel's statistics in numpy fp32, in its order: eight sequential 16-term sums, a sequential sum of
    the eight, mean = total * 2^-7; M2 two-pass about that mean in the same order -- or, two_pass=False, the
    sum-of-squares form sum v^2 - 128 mean^2 that the kernel must not use."""
    seg = y.astype(np.float32).reshape(y.shape[0], -1, 8, 16)

    def total(a):
        part = np.zeros(a.shape[:3], np.float32)
        for j in range(16):
            part = part + a[..., j]
        tot = np.zeros(a.shape[:2], np.float32)
        for s in range(8):
            tot = tot + part[..., s]
        return tot
    mean = total(seg) * np.float32(1.0 / 128.0)
    if two_pass:
        d = seg - mean[:, :, None, None]
        return mean, total(d * d)
    return mean, total(seg * seg) - np.float32(128.0) * mean * mean


@pytest.mark.parametrize("C", [1, 33])
@pytest.mark.parametrize("shift,scale", [(0.0, 1.0), (100.0, 0.1)])
def test_kernel_shaped_statistics_are_inside_the_bounds_and_sum_of_squares_is_not(shift, scale, C):
    k = QC.stack_case("tiles", C, shift, scale, dense=bool(shift))
    _, y = R.query_group_stack_ref(k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"], k["feats"], k["idx"], k["wx"])
    y = _f32(y).double()
    tile_mean, tile_m2, _, _ = R.qg_tile_stats_ref(y)
    dmean, dm2 = R.qg_tile_stats_bounds(y)
    mean, m2 = _tile_stats_fp32(y.numpy(), two_pass=True)
    assert (np.abs(mean - tile_mean.numpy()) <= dmean.numpy()).all()
    assert (np.abs(m2 - tile_m2.numpy()) <= dm2.numpy()).all()
    if shift:                                                 # |mean| >> std: every (channel, tile) cell leaves the bound
        _, naive = _tile_stats_fp32(y.numpy(), two_pass=False)
        assert (np.abs(naive - tile_m2.numpy()) > dm2.numpy()).all()


@pytest.mark.parametrize("name", [n for n in sorted(QC.BATCH_FWD_CASES) if QC.BATCH_FWD_CASES[n][1]])
def test_proj_forward_bound_sees_a_dropped_wx_term(name):
    k = QC.batch_fwd_case(name)
    rel, y = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"], k["wx"])
    _, gathered = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"])
    wx = k["wx"].copy()
    wx[:, 2] = 0
    _, dropped = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"], wx)
    assert ((dropped - y).abs() > R.qg_proj_fwd_bound(gathered, k["wx"], rel)).any()
