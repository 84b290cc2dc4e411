"""Device tests of the inference Voxel-RoI pooling route: the kernel (mgar_voxel_roi_pool_eval_fwd /
mgar_voxel_roi_pool_eval_bf16_fwd, csrc/voxel_roi_pool.hip)
against the float64 reference and per-element bound of voxel_roi_pool_eval_cases.py, its bit repeatability, position independence,
NaN behaviour and -- with an identity epilogue -- bit equality with the train-mode kernel that carries the op-level tests; then the
host route: NeighborVoxelSAModuleMSG fused against switch-off against a float64 truth, which entry points each mode reaches, and
VoxelRCNNHead writing one (M, C_total) buffer.

Measured on an MI355X (max err / bound over all cases, Co and activations): see test_values' docstring."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

import torch_refs as R
import voxel_roi_pool_eval_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASE_IDS = [E.case_id(s, v) for s, v in E.CASES]


def _mods():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as P
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules as V
    return L, P, V


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()               # a copy: the shared cases are read-only
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=4)
def _device_case(size, variant, bf16):
    """The case's tensors on the device; feats inside a wider (N, C + PAD_F) matrix whose surplus columns hold a sentinel."""
    case = E.pooled_ref(size, variant, bf16)[0]
    dt = BF if bf16 else torch.float32
    d = {k: _cuda(case[k]) for k in ("xyz", "new_xyz", "idx_raw", "w_pos", "ps", "pb")}
    wide = torch.full((case["feats"].shape[0], size[2] + E.PAD_F), E.SENTINEL, dtype=dt, device="cuda")
    wide[:, :size[2]] = _cuda(case["feats"], dt)
    d["feats_wide"] = wide
    return d


def _run(P, d, size, co, relu, w_out, scale, shift, feats=None, new_xyz=None, idx=None, pad=E.PAD_OUT):
    """-> the (M, Co + pad) buffer, pre-filled with the sentinel; the kernel writes its first Co columns through ld_out"""
    feats = d["feats_wide"] if feats is None else feats
    new_xyz = d["new_xyz"] if new_xyz is None else new_xyz
    idx = d["idx_raw"] if idx is None else idx
    m = idx.shape[0]
    buf = torch.full((m, co + pad), E.SENTINEL, dtype=feats.dtype, device="cuda")
    P.voxel_roi_pool_eval_fwd(m, size[1], size[2], co, d["xyz"], new_xyz, feats, idx, d["w_pos"], d["ps"], d["pb"], w_out, scale, shift,
                              relu, buf[:, :co])
    torch.cuda.synchronize()
    return buf


def _out_params(size, variant, bf16, co):
    w_out, scale, shift, _ = E.out_params(size, variant, bf16, co)
    return _cuda(w_out), _cuda(scale), _cuda(shift)


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size,variant", E.CASES, ids=CASE_IDS)
def test_values(size, variant, bf16):
    """Every case x payload x Co in {32, 7, 1} x relu in {0, 1}, with ld_f = C + 5 and ld_out = Co + 3, inside the bound of
    voxel_roi_pool_eval_cases.py; the surplus columns of the output keep their sentinel bit for bit, a ReLU never gives -0.
    Measured max err / bound on an MI355X: fp32 0.32, bf16 0.99 (the bf16 bound is one rounding at 2^-8 and is attained next to
    a power of two by construction)."""
    _, P, _ = _mods()
    d = _device_case(size, variant, bf16)
    worst = 0.0
    for co in E.COUTS:
        params = _out_params(size, variant, bf16, co)
        for relu in (0, 1):
            ref, lim = E.reference(size, variant, bf16, co, relu)
            buf = _run(P, d, size, co, relu, *params)
            assert buf.dtype == (BF if bf16 else torch.float32)
            assert (buf[:, co:] == E.SENTINEL).all(), "columns beyond Co were written"
            got = buf[:, :co].double().cpu().numpy()
            assert np.isfinite(got).all()
            used = float((np.abs(got - ref) / lim).max())
            worst = max(worst, used)
            print("%s %s Co %d relu %d: max err / bound = %.3f" % (E.case_id(size, variant), "bf16" if bf16 else "fp32", co, relu, used))
            assert used <= 1.0, (co, relu, used)
            if relu:
                assert (got >= 0).all() and not np.signbit(got).any()
    print("%s %s: worst max err / bound = %.3f" % (E.case_id(size, variant), "bf16" if bf16 else "fp32", worst))


# ---- bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size,variant", E.CASES, ids=CASE_IDS)
def test_bit_repeatable_and_position_independent(size, variant, bf16):
    """The same launch twice gives the same bits; a reversed, strided subset of the queries in a launch of its own -- other M,
    other positions, other workgroup neighbours -- gives the bits of those rows; so does another ld_out."""
    _, P, _ = _mods()
    d = _device_case(size, variant, bf16)
    params = _out_params(size, variant, bf16, 7)
    first = _run(P, d, size, 7, 1, *params)
    again = _run(P, d, size, 7, 1, *params)
    assert torch.equal(first, again)
    sel = torch.arange(size[0] - 1, -1, -3, device="cuda")
    sub = _run(P, d, size, 7, 1, *params, new_xyz=d["new_xyz"][sel].contiguous(), idx=d["idx_raw"][sel].contiguous(), pad=0)
    assert sub.shape[0] == len(sel) and torch.equal(sub, first[sel][:, :7])
    tight = _run(P, d, size, 7, 1, *params, feats=d["feats_wide"][:, :size[2]].contiguous(), pad=0)
    assert torch.equal(tight, first[:, :7])


# ---- NaN ------------------------------------------------------------------------------------------------------------------------
def _torch_chain(d, size, feats, w_out, scale, shift, relu):
    """torch's evaluation of the chain on the device, fp32: gather, position term, max over nsample, ReLU, mlps_out's affine map"""
    idx = d["idx_raw"].long()
    empty = idx[:, 0] < 0
    rows = idx.clamp_min(0).masked_fill(empty[:, None], 0)
    zero = torch.zeros((), device="cuda")
    r = torch.where(empty[:, None, None], zero, d["xyz"][rows] - d["new_xyz"][:, None, :])
    v = torch.where(empty[:, None, None], zero, feats.float()[rows]) + (torch.einsum("msk,ck->msc", r, d["w_pos"]) * d["ps"] + d["pb"])
    pooled = torch.relu(v.max(dim=1).values)
    o = (pooled @ w_out.t()) * scale + shift
    return torch.relu(o) if relu else o


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_nan_reaches_exactly_the_queries_that_name_the_row(bf16):
    """One NaN in one channel of one voxel row: the queries whose idx row names that voxel are NaN in every output (w_out is
    dense; a zero out_scale does not stop a NaN), in the pattern torch's max / relu / matmul give, and every other row keeps
    the bits of the clean run.  The NaN sits in slot 5 of a known query with candidates before and after it: the running max
    must take it and keep it."""
    _, P, _ = _mods()
    size, variant = (180, 16, 16), None
    d = _device_case(size, variant, bf16)
    idx = E.pooled_ref(size, variant, bf16)[0]["idx_raw"]
    full = np.nonzero((idx[:, 0] >= 0) & (idx[:, 5] != idx[:, 0]))[0]          # a query with at least six distinct hits
    q = int(full[0])
    row = int(idx[q, 5])
    named = torch.from_numpy((idx == row).any(axis=1) & (idx[:, 0] >= 0))
    assert named[q] and 0 < int(named.sum()) < size[0]
    feats = d["feats_wide"].clone()
    feats[row, 3] = float("nan")
    for co in (32, 7):
        params = _out_params(size, variant, bf16, co)
        assert (params[1] == 0).any()
        for relu in (0, 1):
            clean = _run(P, d, size, co, relu, *params)
            got = _run(P, d, size, co, relu, *params, feats=feats)
            nan = torch.isnan(got[:, :co]).cpu()
            assert torch.equal(nan, named[:, None].expand(-1, co)), "NaN rows: %s, expected %s" % (
                nan.any(1).nonzero().flatten().tolist(), named.nonzero().flatten().tolist())
            assert torch.equal(got[~named.cuda()], clean[~named.cuda()])
            want = _torch_chain(d, size, feats[:, :size[2]], *params, relu)
            assert torch.equal(torch.isnan(want).cpu(), nan)


# ---- identity epilogue: the gather and the max are the train-mode kernel's -------------------------------------------------------
@pytest.mark.parametrize("size,variant", E.CASES, ids=CASE_IDS)
def test_identity_epilogue_equals_the_train_mode_kernel(size, variant):
    """W_out = I, out_scale = 1, out_shift = 0, relu = 0, Co = C: the fp32 output is bit-equal to the transpose of
    mgar_voxel_roi_pool_fwd's pooled, called with mean = 0, invstd = 1, gamma = ps, beta = pb.  That kernel forms
    (p - 0) * (1 * ps) + pb in two roundings, the new one fmaf(p, ps, pb) in one; with ps a signed power of two the product is
    exact and both are the same fp32 expression (the case's ps is replaced by sign(ps) 2^round(log2 |ps|), pb kept)."""
    _, P, _ = _mods()
    d = _device_case(size, variant, False)
    m, ns, c = size
    ps = torch.sign(d["ps"]) * torch.exp2(torch.round(torch.log2(d["ps"].abs())))
    assert (ps != 0).all() and torch.equal(torch.frexp(ps.abs())[0], torch.full_like(ps, 0.5))
    feats = d["feats_wide"][:, :c].contiguous()
    pooled = torch.full((c, m), -3.0, device="cuda")
    arg = torch.zeros((c, m), dtype=torch.uint8, device="cuda")
    P.voxel_roi_pool_fwd(m, ns, c, d["xyz"], d["new_xyz"], feats, d["idx_raw"], d["w_pos"], torch.zeros(c, device="cuda"),
                         torch.ones(c, device="cuda"), ps, d["pb"], pooled, arg)
    out = torch.full((m, c), -3.0, device="cuda")
    P.voxel_roi_pool_eval_fwd(m, ns, c, c, d["xyz"], d["new_xyz"], feats, d["idx_raw"], d["w_pos"], ps, d["pb"], torch.eye(c, device="cuda"),
                              torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"), 0, out)
    torch.cuda.synchronize()
    assert torch.equal(out, pooled.t()) and (out >= 0).all()
    if variant is None and m >= 180:
        assert (out > 0).any() and (out == 0).any()


def test_refusals_raise_and_an_empty_launch_writes_nothing():
    L, P, _ = _mods()
    size = (180, 16, 16)
    d = _device_case(size, None, False)
    params = _out_params(size, None, False, 7)
    buf = torch.full((180, 10), E.SENTINEL, device="cuda")
    args = lambda m, c, co, out: (m, 16, c, co, d["xyz"], d["new_xyz"], d["feats_wide"], d["idx_raw"], d["w_pos"], d["ps"], d["pb"],   # noqa: E731
                                  params[0], params[1], params[2], 1, out)
    with pytest.raises(L.MgarError):
        P.voxel_roi_pool_eval_fwd(*args(180, 16, 7, buf[:, :6]))                # out is not (M, Co)
    with pytest.raises(L.MgarError):
        P.voxel_roi_pool_eval_fwd(*args(180, 22, 7, buf[:, :7]))                # feats has 21 columns
    with pytest.raises(L.MgarError):
        P.voxel_roi_pool_eval_fwd(*args(180, 16, 7, buf.t()[:7].t().double()))  # dtype
    P.voxel_roi_pool_eval_fwd(*args(0, 16, 7, buf[:0, :7]))
    torch.cuda.synchronize()
    assert (buf == E.SENTINEL).all()


# ---- the module -----------------------------------------------------------------------------------------------------------------
N_QUERY = 4096          # x 32 output channels: 1.3e5 entries


@functools.lru_cache(maxsize=None)
def _grid(c_in):
    """A voxel_roi_pool_cases.make_case-style grid for the module: 8 x 64 x 64 cells of 0.25 x 0.25 x 0.5 m, 30 % occupied in
    random row order, continuous random queries of which 3 % lie far outside.  -> host tensors"""
    rng = np.random.default_rng([3, c_in])
    Z, Y, X = 8, 64, 64
    voxel, lo = np.array([0.25, 0.25, 0.5]), np.array([-8.0, -8.0, -2.0])
    z, y, x = np.nonzero(rng.random((Z, Y, X)) < 0.30)
    perm = rng.permutation(len(z))
    zyx = np.stack([z[perm], y[perm], x[perm]], 1)
    xyz = ((zyx[:, ::-1] + 0.5) * voxel + lo).astype(np.float32)
    v2p = -np.ones((1, Z, Y, X), np.int32)
    v2p[0, zyx[:, 0], zyx[:, 1], zyx[:, 2]] = np.arange(len(zyx), dtype=np.int32)
    q = lo + rng.random((N_QUERY, 3)) * np.array([X, Y, Z]) * voxel
    q[rng.permutation(N_QUERY)[:int(0.03 * N_QUERY)]] += 40.0
    new_xyz = q.astype(np.float32)
    cell = np.floor((new_xyz.astype(np.float64) - lo) / voxel).astype(np.int32)                  # (x, y, z)
    coords = np.concatenate([np.zeros((N_QUERY, 1), np.int32), cell], 1)                         # [b, x, y, z]
    feats = rng.standard_normal((len(zyx), c_in)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (xyz, new_xyz, coords, feats, v2p))


def _module(c_in, seed=0):
    _, _, V = _mods()
    mod = V.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2]], radii=[0.75], nsamples=[16], mlps=[[c_in, 32, 32]])
    return fill_deterministic(mod, seed=seed).eval().cuda()       # running statistics perturbed: mean 0.1 N(0, 1), var U(0.5, 1.5)


def _forward(mod, c_in, dtype=torch.float32, autocast=False, **kw):
    xyz, new_xyz, coords, feats, v2p = (t.cuda() for t in _grid(c_in))
    with torch.autocast("cuda", dtype=BF, enabled=autocast):
        out = mod(xyz=xyz, xyz_batch_cnt=torch.tensor([xyz.shape[0]], dtype=torch.int32, device="cuda"), new_xyz=new_xyz,
                  new_xyz_batch_cnt=torch.tensor([N_QUERY], dtype=torch.int32, device="cuda"), new_coords=coords,
                  features=feats.to(dtype), voxel2point_indices=v2p, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _truth(c_in):
    """float64: eval-mode mlps_in on all voxels, voxel_roi_pool_ref on the indices the device query wrote, mlps_out -- assembled
    from the module's parameters with float64 matmuls."""
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_query_utils
    mod = _module(c_in).cpu().double()
    xyz, new_xyz, coords, feats, v2p = _grid(c_in)
    g = mod.groupers[0]
    idx = voxel_query_utils.voxel_query_raw(g.max_range, g.radius, g.nsample, xyz.cuda(), new_xyz.cuda(),
                                            coords[:, [0, 3, 2, 1]].contiguous().cuda(), v2p.cuda()).cpu()

    def bn_eval(bn, x):       # x (n, C)
        return (x - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps) * bn.weight + bn.bias
    with torch.no_grad():
        conv_in, bn_in = mod.mlps_in[0][0], mod.mlps_in[0][1]
        pos_conv, pos_bn = mod.mlps_pos[0][0], mod.mlps_pos[0][1]
        conv_out, bn_out = mod.mlps_out[0][0], mod.mlps_out[0][1]
        feats_in = bn_eval(bn_in, feats.double() @ conv_in.weight.view(32, c_in).t())
        ref = R.voxel_roi_pool_ref(xyz, new_xyz, feats_in, idx, pos_conv.weight.view(32, 3), pos_bn.weight, pos_bn.bias, pos_bn.eps, False,
                                   pos_bn.running_mean, pos_bn.running_var)
        return torch.relu(bn_eval(bn_out, ref.pooled.t() @ conv_out.weight.view(32, 32).t())), (idx[:, 0] < 0)


@pytest.mark.parametrize("c_in", [32, 64])
def test_module_fused_against_switch_off_against_float64(c_in, monkeypatch):
    """mil3's pool layers ([[32, 32, 32]] and [[64, 32, 32]]) in .eval() with perturbed running statistics.  fp32: both routes
    within 1e-4 of max |truth| and fused <= max(1.5 x unfused, 1e-6 max |truth|).  bf16 rows under autocast:
    the relative rms distance to the fp32 run satisfies fused <= unfused (strictly fewer roundings, 1.3e5 entries).
    Measured on an MI355X: fp32 error fused / unfused 1.9e-6 / 2.0e-6 and 2.3e-6 / 2.5e-6 at max |truth| 5.8;
    bf16 distance fused / unfused 2.94e-3 / 4.67e-3 and 2.97e-3 / 4.71e-3, ratio 0.63 for both specs."""
    _, _, V = _mods()
    truth, empty = _truth(c_in)
    assert 0 < int(empty.sum()) < N_QUERY and (truth > 0).any() and (truth == 0).any()
    scale = truth.abs().max().item()
    mod = _module(c_in)
    runs = {}
    for fuse in (True, False):
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", fuse)
        with torch.no_grad():
            runs[fuse, "fp32"] = _forward(mod, c_in)
            runs[fuse, "bf16"] = _forward(mod, c_in, BF, autocast=True)
        assert runs[fuse, "fp32"].shape == (N_QUERY, 32) and runs[fuse, "fp32"].dtype == torch.float32
    assert runs[True, "bf16"].dtype == BF and runs[True, "fp32"].is_contiguous()
    err = {fuse: (runs[fuse, "fp32"].double().cpu() - truth).abs().max().item() for fuse in (True, False)}
    print("C_in %d fp32: fused err %.3e, unfused err %.3e, max |truth| %.3e" % (c_in, err[True], err[False], scale))
    assert err[True] <= 1e-4 * scale and err[False] <= 1e-4 * scale
    assert err[True] <= max(1.5 * err[False], 1e-6 * scale)
    yard = runs[False, "fp32"].double()
    dist = {fuse: ((runs[fuse, "bf16"].double() - yard).pow(2).mean().sqrt() / yard.pow(2).mean().sqrt()).item() for fuse in (True, False)}
    print("C_in %d bf16: rel rms distance to fp32 fused %.3e, unfused %.3e, ratio %.3f" % (c_in, dist[True], dist[False],
                                                                                          dist[True] / dist[False]))
    assert dist[True] <= dist[False]


def test_module_out_argument_and_column_slices(monkeypatch):
    """`out`: a column slice of a wider buffer is written in place and returned, its neighbours untouched; the same bits as the
    module's own allocation -- on the fused route directly, with the switch off through a copy."""
    _, _, V = _mods()
    mod = _module(32)
    for fuse in (True, False):
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", fuse)
        with torch.no_grad():
            own = _forward(mod, 32)
            buf = torch.full((N_QUERY, 96), E.SENTINEL, device="cuda")
            got = _forward(mod, 32, out=buf[:, 32:64])
        assert got.data_ptr() == buf[:, 32:64].data_ptr() and torch.equal(got, own)
        assert (buf[:, :32] == E.SENTINEL).all() and (buf[:, 64:] == E.SENTINEL).all()
    with torch.no_grad(), pytest.raises(ValueError):
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
        _forward(mod, 32, out=torch.empty((N_QUERY, 31), device="cuda"))


# ---- routing --------------------------------------------------------------------------------------------------------------------
def _census(monkeypatch, fn):
    """entry points of the library reached while fn() runs -> ({name: calls}, fn's result)"""
    L, _, _ = _mods()
    calls, inner = {}, L.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return inner(name, *a)
    monkeypatch.setattr(L, "call", counting)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(L, "call", inner)
    return calls, out


def _old_and_new(calls):
    new = sum(n for k, n in calls.items() if k in ("mgar_voxel_roi_pool_eval_fwd", "mgar_voxel_roi_pool_eval_bf16_fwd"))
    old = sum(n for k, n in calls.items() if k in ("mgar_voxel_roi_pool_fwd", "mgar_voxel_roi_pool_fwd_bf16"))
    return old, new, sum(n for k, n in calls.items() if k.startswith("mgar_bn"))


def test_routing(monkeypatch):
    """Eval + no_grad reaches the new entry once per scale and neither the train-mode kernel nor a BatchNorm entry; train mode, a
    required gradient and the switch off each reach the old entry and never the new one, with the bits of a run with the
    route disabled."""
    _, _, V = _mods()
    two = V.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2], [1, 2, 2]], radii=[0.75, 0.5], nsamples=[16, 8], mlps=[[32, 32, 32], [32, 16, 7]])
    two = fill_deterministic(two, seed=2).eval().cuda()
    monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
    with torch.no_grad():
        calls, out = _census(monkeypatch, lambda: _forward(two, 32))
        assert calls.get("mgar_voxel_roi_pool_eval_fwd") == 2 and _old_and_new(calls) == (0, 2, 0) and out.shape == (N_QUERY, 39)
        calls, out = _census(monkeypatch, lambda: _forward(two, 32, BF, autocast=True))
        assert calls.get("mgar_voxel_roi_pool_eval_bf16_fwd") == 2 and _old_and_new(calls) == (0, 2, 0) and out.dtype == BF
        # one scale's BatchNorm in train mode: that scale alone keeps the old kernels
        mixed = copy.deepcopy(two)
        mixed.mlps_out[1][1].train()
        calls, out = _census(monkeypatch, lambda: _forward(mixed, 32))
        assert _old_and_new(calls)[:2] == (1, 1) and out.shape == (N_QUERY, 39)

    def both(make, run):
        """run(module) with the route enabled and disabled, on fresh copies -> census of the enabled run; asserts equal bits"""
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
        calls, on = _census(monkeypatch, lambda: run(make()))
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", False)
        off = run(make())
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", True)
        assert torch.equal(on, off)
        return calls

    def no_grad(mod):
        with torch.no_grad():
            return _forward(mod, 32)
    calls = both(lambda: copy.deepcopy(two).train(), no_grad)                                  # train mode
    old, new, _ = _old_and_new(calls)
    assert (old, new) == (2, 0)
    calls = both(lambda: copy.deepcopy(two), lambda mod: _forward(mod, 32).detach())           # eval, but the parameters want a gradient
    assert _old_and_new(calls)[:2] == (2, 0)
    monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", False)                                        # the switch
    with torch.no_grad():
        calls, _ = _census(monkeypatch, lambda: _forward(two, 32))
    assert _old_and_new(calls)[:2] == (2, 0)


# ---- the head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [None, [3, 1]], ids=["all_boxes", "roi_counts"])
def test_head_writes_one_buffer(counts, monkeypatch):
    """VoxelRCNNHead.eval() behind the trunk on two synthetic samples of four boxes: pooled_features has the shape of the
    switch-off run, is contiguous (one (M, 96) buffer, no concatenation) and within the fp32 bar of it; so is shared_feature."""
    from multimodal_gar_amd import synthetic as S, workload as W
    from multimodal_gar_amd.pcdet.models import build_network
    _, _, V = _mods()
    ds = W.SyntheticDataset()
    sc = S.scene_batch(5, 2, 4, 4096)
    pts = torch.from_numpy(np.ascontiguousarray(sc["points"])).cuda()
    b3 = torch.from_numpy(sc["bboxes3d"])[:, :4, :].contiguous().cuda()
    net = fill_deterministic(build_network(W.lidar_model_cfg(4096, "voxel"), 1, ds), seed=9).eval().cuda()
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(V, "MGAR_VRP_EVAL_FUSE", fuse)
        data = W.voxelize_batch(pts, ds)
        data["gt_boxes"] = b3
        if counts is not None:
            data["roi_counts"] = counts
        with torch.no_grad():
            calls, out = _census(monkeypatch, lambda: net(data))
        torch.cuda.synchronize()
        res[fuse] = (out["pooled_features"], out["shared_feature"])
        assert _old_and_new(calls)[:2] == ((0, 3) if fuse else (3, 0))
    rows = sum(counts) if counts is not None else 8
    for k, what in enumerate(("pooled_features", "shared_feature")):
        on, off = res[True][k], res[False][k]
        assert on.shape == off.shape and on.shape[0] == rows and on.dtype == off.dtype == torch.float32, what
        scale, err = off.abs().max().item(), (on - off).abs().max().item()
        print("%s: err %.3e, scale %.3e" % (what, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, what
    assert res[True][0].shape[1:] == (216, 96) and res[True][0].is_contiguous()
