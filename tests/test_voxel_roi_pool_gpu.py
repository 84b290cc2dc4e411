"""Op-level tests of the fused Voxel-RoI pooling kernels (csrc/voxel_roi_pool.hip: mgar_voxel_roi_pool_stats / _fwd /
_fwd_bf16 / _bwd and the two workspace queries) against `torch_refs.voxel_roi_pool_ref`, the reference's op chain
(voxel_pool_modules.py:86-126) restated in float64 with MEASURED BatchNorm statistics and autograd -- the kernels replace
those by closed forms (moments of the relative coordinates; five per-channel sums in the backward).

Every comparison is in the max-norm relative to max |reference|, bound 1e-4 (north_star) unless stated, and goes through
`record_error`.  The inputs come from voxel_roi_pool_cases.py; tests/test_voxel_roi_pool_cpu.py verifies without a kernel
that the closed forms are exact algebra, that the restated chain is the reference project's, and that near-ties (the only
entries exempt from the arg-max comparison, decided from the reference alone) are below 0.5 % of every case.

The backward is tested DECOUPLED from the forward: it is handed the reference's mean / invstd / pooled (rounded to fp32),
moments (double) and first arg-max slot, so no tie decision of the forward kernel can leak into it and nothing is masked.
d w_pos in train mode is a difference of large sums (S2 - S0 E[r] - S1 invstd Cov w); it is bounded the way
test_fusion_ops_gpu.py::test_gatv2_fwd_bwd bounds its parameter gradients: err <= max(1e-5 + 1e-4 scale, 3 err32), err32
being the error of an fp32 torch autograd evaluation of the same chain against float64."""
import functools

import numpy as np
import pytest
import torch

import torch_refs as R
import voxel_roi_pool_cases as VC
from conftest import record_error

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF = torch.bfloat16

FULL = [(s, None) for s in VC.FULL_SIZES] + [(VC.ALL_EMPTY, "all_empty")]
COND = [(VC.CONDITIONING_SIZE, v) for v in VC.CONDITIONING]


def _ids(cases):
    return ["%s%s" % (VC.size_id(s), "_" + v if v else "") for s, v in cases]


def _mods():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as P
    return L, P


@functools.lru_cache(maxsize=4)
def _case(size, variant):
    return VC.make_case(*size, variant=variant)


def _dev(case):
    return {k: torch.from_numpy(v).cuda() for k, v in case.items() if isinstance(v, np.ndarray)}


def _cmp(what, got, want, tol=TOL):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.numel() == 0:
        return
    assert torch.isfinite(got).all(), what
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    record_error(what, err, scale, tol)
    print("%-28s err %.3e  scale %.3e  rel %.3e" % (what, err, scale, err / max(scale, 1e-300)))
    assert err <= tol * scale, "%s: max err %g vs scale %g (rel %.3e > %g)" % (what, err, scale, err / max(scale, 1e-300), tol)


def _cmp_dw(what, got, want, want32):
    """d w_pos: err <= max(1e-5 + 1e-4 scale, 3 err32) (module docstring)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    err32 = (want32.detach().double().cpu() - want).abs().max().item()
    record_error(what, err, scale, TOL)
    print("%-28s err %.3e  scale %.3e  rel %.3e  torch-fp32 err %.3e" % (what, err, scale, err / max(scale, 1e-300), err32))
    assert err <= max(1e-5 + TOL * scale, 3.0 * err32), "%s: err %g, torch-fp32 err %g, scale %g" % (what, err, err32, scale)


def _invstd(ref, eps):
    return 1.0 / torch.sqrt(ref.var.detach() + eps)


# ------------------------------------------------------------------------------------------------------------- stats
def _run_stats(P, d, case, rm, rv, nbt):
    m, ns, c = case["M"], case["nsample"], case["C"]
    mean, invstd = torch.full((c,), 7.0, device="cuda"), torch.full((c,), 7.0, device="cuda")
    moments = torch.full((10,), 7.0, dtype=torch.float64, device="cuda")
    P.voxel_roi_pool_stats(m, ns, c, d["xyz"], d["new_xyz"], d["idx_raw"], d["w_pos"], case["eps"], 0.1, moments, mean, invstd,
                           rm, rv, nbt)
    torch.cuda.synchronize()
    return mean, invstd, moments


STATS = FULL + [(VC.CAP_CASE, None)] + COND


@pytest.mark.parametrize("size,variant", STATS, ids=_ids(STATS))
def test_stats_match_the_measured_statistics(size, variant):
    """mean / invstd / the ten moments against statistics MEASURED on p = w_pos . r in float64; the running buffers after
    two consecutive calls (momentum applied twice; the unbiased factor n / (n - 1) is 25 % at n = 5 and undefined at
    n = 1, where the biased value is kept); NULL running buffers; same bits on a second run."""
    _, P = _mods()
    case = _case(size, variant)
    d = _dev(case)
    ref1 = VC.reference(case, stats_only=True)[0]
    if variant == "one_sided":
        r = ref1.r.reshape(-1, 3)
        print("one-sided: max_axis |E[r]| / std(r) = %.2f" % (r.mean(0).abs() / r.std(0, unbiased=False)).max().item())
    ref2 = R.voxel_roi_pool_ref(torch.from_numpy(case["xyz"]), torch.from_numpy(case["new_xyz"]), None,
                                torch.from_numpy(case["idx_raw"]), torch.from_numpy(case["w_pos"]), None, None, case["eps"], True,
                                ref1.running_mean, ref1.running_var)
    rm, rv = d["running_mean"].clone(), d["running_var"].clone()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    first = _run_stats(P, d, case, rm, rv, nbt)
    rm1, rv1 = rm.clone(), rv.clone()
    mean, invstd, moments = _run_stats(P, d, case, rm, rv, nbt)
    for a, b in zip(first, (mean, invstd, moments)):
        assert torch.equal(a, b)
    assert nbt.item() == 2
    _cmp("stats/mean", mean, ref1.mean)
    _cmp("stats/invstd", invstd, _invstd(ref1, case["eps"]))
    _cmp("stats/moments_E[r]", moments[:3], ref1.moments[:3])
    _cmp("stats/moments_Cov(r)", moments[3:9], ref1.moments[3:9])
    assert moments[9].item() == float(size[0] * size[1])
    _cmp("stats/running_mean_1", rm1, ref1.running_mean)
    _cmp("stats/running_var_1", rv1, ref1.running_var)
    _cmp("stats/running_mean_2", rm, ref2.running_mean)
    _cmp("stats/running_var_2", rv, ref2.running_var)
    # a second run from the same buffers gives the same bits; NULL running buffers are accepted
    rm_b, rv_b = d["running_mean"].clone(), d["running_var"].clone()
    again = _run_stats(P, d, case, rm_b, rv_b, None)
    bare = _run_stats(P, d, case, None, None, None)
    for a, b, c in zip(first, again, bare):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(rm_b, rm1) and torch.equal(rv_b, rv1)


# ----------------------------------------------------------------------------------------------------------- forward
def _run_fwd(P, d, case, ref, feats, gamma, beta):
    m, ns, c = case["M"], case["nsample"], case["C"]
    pooled = torch.full((c, m), -3.0, dtype=feats.dtype, device="cuda")
    arg = torch.full((c, m), 201, dtype=torch.uint8, device="cuda")
    P.voxel_roi_pool_fwd(m, ns, c, d["xyz"], d["new_xyz"], feats, d["idx_raw"], d["w_pos"], ref.mean.detach().float().cuda(),
                         _invstd(ref, case["eps"]).float().cuda(), gamma, beta, pooled, arg)
    torch.cuda.synchronize()
    return pooled, arg


def _check_fwd(tag, case, ref, pooled, arg, gamma, beta):
    idx = torch.from_numpy(case["idx_raw"])
    _cmp(tag + "/pooled", pooled, ref.pooled)
    mask = R.near_tie_mask(ref.pre, idx, VC.NEAR_TIE_MARGIN)
    live = idx[:, 0] != -1
    assert mask.sum().item() <= VC.NEAR_TIE_CAP * max(live.sum().item() * case["C"], 1)
    got = arg.t().cpu().long()
    assert torch.equal(got[~mask], ref.arg[~mask]), "%s: %d arg-max slots differ outside the near-tie mask" % (
        tag, (got[~mask] != ref.arg[~mask]).sum().item())
    if (~live).any():       # empty neighbourhoods: slot 0 and relu(BN(0)) in every channel
        assert (got[~live] == 0).all()
        bn0 = -ref.mean.detach() * _invstd(ref, case["eps"])
        bn0 = bn0 * (1.0 if gamma is None else torch.from_numpy(case["gamma"]).double())
        bn0 = bn0 + (0.0 if beta is None else torch.from_numpy(case["beta"]).double())
        want = torch.relu(bn0)[:, None].expand(-1, int((~live).sum()))
        _cmp(tag + "/pooled_empty_rows", pooled.cpu()[:, ~live], want)


@pytest.mark.parametrize("size,variant", FULL + COND, ids=_ids(FULL + COND))
def test_forward_fp32(size, variant):
    """pooled and the first arg-max slot; then the same through a feature matrix with ld_f = C + 5 (same bits), and with
    gamma / beta NULL (no affine)."""
    _, P = _mods()
    case = _case(size, variant)
    d = _dev(case)
    ref = VC.reference(case)[0]
    pooled, arg = _run_fwd(P, d, case, ref, d["feats"], d["gamma"], d["beta"])
    _check_fwd("fwd", case, ref, pooled, arg, d["gamma"], d["beta"])
    wide = torch.randn((d["feats"].shape[0], size[2] + 5), device="cuda")
    wide[:, :size[2]] = d["feats"]
    pooled_w, arg_w = _run_fwd(P, d, case, ref, wide, d["gamma"], d["beta"])
    assert torch.equal(pooled_w, pooled) and torch.equal(arg_w, arg)
    ref_na = VC.reference(case, affine=False)[0]
    pooled_na, arg_na = _run_fwd(P, d, case, ref_na, d["feats"], None, None)
    _check_fwd("fwd_no_affine", case, ref_na, pooled_na, arg_na, None, None)


@pytest.mark.parametrize("size,variant", FULL, ids=_ids(FULL))
def test_forward_bf16_equals_rounded_fp32(size, variant):
    """The project's bf16 convention (tests/test_bf16_gpu.py): the bf16 twin computes in fp32 on the bf16 payload and rounds
    once -- bit-equal to the fp32 kernel on the bf16-rounded features, rounded to bf16; identical arg-max."""
    _, P = _mods()
    case = _case(size, variant)
    d = _dev(case)
    ref = VC.reference(case, stats_only=True)[0]
    fb = d["feats"].to(BF)
    p16, a16 = _run_fwd(P, d, case, ref, fb, d["gamma"], d["beta"])
    p32, a32 = _run_fwd(P, d, case, ref, fb.float(), d["gamma"], d["beta"])
    assert p16.dtype == BF and torch.equal(p16, p32.to(BF)) and torch.equal(a16, a32)


# ---------------------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=2)
def _bwd_reference(size, variant, train, unit_affine):
    """Float64 chain + autograd (and its fp32 twin, for the d w_pos yardstick) -> reference namespace and gradients."""
    case = _case(size, variant)
    if unit_affine:     # what a NULL gamma means: gamma = 1 (beta is not an input of the backward)
        case = dict(case, gamma=np.ones_like(case["gamma"]))
    cot = torch.from_numpy(case["cot"])
    ref, feats, w, gamma, beta = VC.reference(case, train=train, requires_grad=True)
    (ref.pooled * cot.double()).sum().backward()
    ref32, _, w32, _, _ = VC.reference(case, train=train, requires_grad=True, dtype=torch.float32)
    (ref32.pooled * cot).sum().backward()
    ref.pre = None      # (M, C, nsample) doubles: not needed by the backward tests
    return case, ref, feats.grad, w.grad, gamma.grad, beta.grad, w32.grad


def _run_bwd(P, d, case, ref, train, gamma, dfeats):
    m, ns, c = case["M"], case["nsample"], case["C"]
    dgamma, dbeta = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    dw = torch.full((c, 3), float("nan"), device="cuda")
    P.voxel_roi_pool_bwd(m, ns, c, d["xyz"], d["new_xyz"], d["idx_raw"], d["w_pos"], ref.mean.detach().float().cuda(),
                         _invstd(ref, case["eps"]).float().cuda(), gamma, ref.moments.cuda() if train else None, int(train), d["cot"],
                         ref.pooled.detach().float().contiguous().cuda(), ref.arg.t().contiguous().to(torch.uint8).cuda(), dfeats,
                         dgamma, dbeta, dw)
    torch.cuda.synchronize()
    return dgamma, dbeta, dw


@pytest.mark.parametrize("train", [True, False], ids=["train_stats", "eval_stats"])
@pytest.mark.parametrize("size,variant", FULL, ids=_ids(FULL))
def test_backward_decoupled_from_the_forward(size, variant, train):
    _, P = _mods()
    case, ref, dfeats_ref, dw_ref, dgamma_ref, dbeta_ref, dw32 = _bwd_reference(size, variant, train, False)
    d = _dev(case)
    dfeats = torch.zeros_like(d["feats"])
    dgamma, dbeta, dw = _run_bwd(P, d, case, ref, train, d["gamma"], dfeats)
    _cmp("bwd/dfeats", dfeats, dfeats_ref)
    _cmp("bwd/dgamma", dgamma, dgamma_ref)
    _cmp("bwd/dbeta", dbeta, dbeta_ref)
    _cmp_dw("bwd/dw_pos", dw, dw_ref, dw32)
    # fixed-order sums: a second run gives the same bits (dfeats goes through float atomics and is not asserted bitwise)
    again = _run_bwd(P, d, case, ref, train, d["gamma"], torch.zeros_like(d["feats"]))
    for a, b in zip((dgamma, dbeta, dw), again):
        assert torch.equal(a, b)


VARIANT_SIZES = [((2117, 16, 32), None), ((333, 1, 1), None), ((130, 255, 5), None)]


@pytest.mark.parametrize("train", [True, False], ids=["train_stats", "eval_stats"])
@pytest.mark.parametrize("size,variant", VARIANT_SIZES, ids=_ids(VARIANT_SIZES))
def test_backward_null_and_strided_arguments(size, variant, train):
    """gamma NULL (= 1); dfeats NULL; dfeats with ld_f = C + 5, pre-filled: accumulated into, extra columns untouched."""
    _, P = _mods()
    case, ref, dfeats_ref, dw_ref, dgamma_ref, dbeta_ref, dw32 = _bwd_reference(size, variant, train, True)
    d = _dev(case)
    dfeats = torch.zeros_like(d["feats"])
    dgamma, dbeta, dw = _run_bwd(P, d, case, ref, train, None, dfeats)
    _cmp("bwd_gamma_null/dfeats", dfeats, dfeats_ref)
    _cmp("bwd_gamma_null/dgamma", dgamma, dgamma_ref)
    _cmp("bwd_gamma_null/dbeta", dbeta, dbeta_ref)
    _cmp_dw("bwd_gamma_null/dw_pos", dw, dw_ref, dw32)

    case, ref, dfeats_ref, dw_ref, dgamma_ref, dbeta_ref, dw32 = _bwd_reference(size, variant, train, False)
    d = _dev(case)
    plain = _run_bwd(P, d, case, ref, train, d["gamma"], torch.zeros_like(d["feats"]))
    none = _run_bwd(P, d, case, ref, train, d["gamma"], None)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    _cmp("bwd_dfeats_null/dgamma", none[0], dgamma_ref)
    _cmp("bwd_dfeats_null/dbeta", none[1], dbeta_ref)
    _cmp_dw("bwd_dfeats_null/dw_pos", none[2], dw_ref, dw32)

    c = size[2]
    n_rows = d["feats"].shape[0]
    pattern = (torch.arange(n_rows * (c + 5), device="cuda", dtype=torch.float32).view(n_rows, c + 5) % 7.0) * 0.25 - 0.5
    wide = pattern.clone()
    strided = _run_bwd(P, d, case, ref, train, d["gamma"], wide)
    for a, b in zip(plain, strided):
        assert torch.equal(a, b)
    assert torch.equal(wide[:, c:], pattern[:, c:])
    _cmp("bwd_wide/dfeats", wide[:, :c].double() - pattern[:, :c].double(), dfeats_ref)


# -------------------------------------------------------------------------------------------------- autograd function
@pytest.mark.parametrize("train", [True, False], ids=["bn_train", "bn_eval"])
@pytest.mark.parametrize("size,variant", FULL, ids=_ids(FULL))
def test_autograd_function_forward_and_backward(size, variant, train):
    """_FusedVoxelRoIPool (stats -> fwd -> bwd on the kernels' own intermediates) against the chain.  The cotangent is
    zeroed where the forward may legitimately decide differently from float64: near-ties between different voxel rows,
    and best values within the same margin of the ReLU's kink -- both masks come from the reference alone."""
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import _FusedVoxelRoIPool
    case = _case(size, variant)
    d = _dev(case)
    c = size[2]
    ref, feats64, w64, gamma64, beta64 = VC.reference(case, train=train, requires_grad=True)
    idx = torch.from_numpy(case["idx_raw"])
    best = ref.pre.detach().max(dim=2).values
    mask = R.near_tie_mask(ref.pre, idx, VC.NEAR_TIE_MARGIN) | (best.abs() < VC.NEAR_TIE_MARGIN * ref.pre.detach().abs().max())
    cot = torch.from_numpy(case["cot"]) * (~mask).t()
    (ref.pooled * cot.double()).sum().backward()
    ref32, _, w32, _, _ = VC.reference(case, train=train, requires_grad=True, dtype=torch.float32)
    (ref32.pooled * cot).sum().backward()

    bn = torch.nn.BatchNorm2d(c, eps=case["eps"]).cuda()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
        bn.running_mean.copy_(d["running_mean"]); bn.running_var.copy_(d["running_var"])
    bn.train(train)
    feats, w = d["feats"].clone().requires_grad_(True), d["w_pos"].clone().requires_grad_(True)
    pooled, arg = _FusedVoxelRoIPool.apply(d["xyz"], d["new_xyz"], feats, d["idx_raw"], w, bn.weight, bn.bias, bn)
    (pooled * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    _cmp("fn/pooled", pooled, ref.pooled)
    got = arg.t().cpu().long()
    assert torch.equal(got[~mask], ref.arg[~mask])
    _cmp("fn/dfeats", feats.grad, feats64.grad)
    _cmp("fn/dgamma", bn.weight.grad, gamma64.grad)
    _cmp("fn/dbeta", bn.bias.grad, beta64.grad)
    _cmp_dw("fn/dw_pos", w.grad, w64.grad, w32.grad)
    if train:
        _cmp("fn/running_mean", bn.running_mean, ref.running_mean)
        _cmp("fn/running_var", bn.running_var, ref.running_var)
        assert bn.num_batches_tracked.item() == 1
    else:
        assert torch.equal(bn.running_mean, d["running_mean"]) and torch.equal(bn.running_var, d["running_var"])
        assert bn.num_batches_tracked.item() == 0


# --------------------------------------------------------------------------------------------------------- arguments
def test_bad_sizes_raise_and_empty_calls_touch_nothing():
    L, P = _mods()
    case = _case((180, 16, 16), None)
    d = _dev(case)
    m, ns, c = 180, 16, 16
    n_rows = d["feats"].shape[0]
    st = L.stream_of(d["xyz"])
    f32 = lambda *shape: torch.full(shape, 5.0, device="cuda")                     # noqa: E731
    mean, invstd, moments = f32(c), f32(c), torch.full((10,), 5.0, dtype=torch.float64, device="cuda")
    rm, rv, nbt = f32(c), f32(c), torch.full((), 5, dtype=torch.int64, device="cuda")
    ws_d = torch.zeros((2048 * 9,), dtype=torch.float64, device="cuda")
    ws_f = torch.zeros((64 * 33 * 5,), device="cuda")
    wide_feats = torch.zeros((n_rows, 40), device="cuda")
    pooled, arg = f32(40, m), torch.full((40, m), 5, dtype=torch.uint8, device="cuda")
    dfeats, dgamma, dbeta, dw = f32(n_rows, 40), f32(40), f32(40), f32(40, 3)
    w40 = torch.zeros((40, 3), device="cuda")

    def stats(m_, ns_, c_):
        return L.call("mgar_voxel_roi_pool_stats", m_, ns_, c_, L.fptr(d["xyz"]), L.fptr(d["new_xyz"]), L.iptr(d["idx_raw"]), L.fptr(w40),
                      1e-5, 0.1, L.dev_ptr(ws_d), L.dev_ptr(moments), L.fptr(mean), L.fptr(invstd), L.fptr(rm), L.fptr(rv),
                      L.dev_ptr(nbt), st)

    def fwd(name, m_, ns_, c_, ld):
        dt = BF if name.endswith("bf16") else torch.float32
        return L.call(name, m_, ns_, c_, L.fptr(d["xyz"]), L.fptr(d["new_xyz"]), L.dev_ptr(wide_feats.to(dt)), ld, L.iptr(d["idx_raw"]),
                      L.fptr(w40), L.fptr(f32(40)), L.fptr(f32(40)), L.fptr(f32(40)), L.fptr(f32(40)), L.dev_ptr(pooled.to(dt)),
                      L.dev_ptr(arg), st)

    def bwd(m_, ns_, c_, ld):
        return L.call("mgar_voxel_roi_pool_bwd", m_, ns_, c_, L.fptr(d["xyz"]), L.fptr(d["new_xyz"]), L.iptr(d["idx_raw"]), L.fptr(w40),
                      L.fptr(f32(40)), L.fptr(f32(40)), L.fptr(f32(40)), L.dev_ptr(moments), 1, L.fptr(f32(40, m)), L.fptr(f32(40, m)),
                      L.dev_ptr(arg), L.fptr(ws_f), L.fptr(dfeats), ld, L.fptr(dgamma), L.fptr(dbeta), L.fptr(dw), st)

    for bad_c in (0, 33):
        with pytest.raises(L.MgarError):
            stats(m, ns, bad_c)
        with pytest.raises(L.MgarError):
            bwd(m, ns, bad_c, 40)
        for name in ("mgar_voxel_roi_pool_fwd", "mgar_voxel_roi_pool_fwd_bf16"):
            with pytest.raises(L.MgarError):
                fwd(name, m, ns, bad_c, 40)
    with pytest.raises(L.MgarError):
        stats(m, 0, c)
    with pytest.raises(L.MgarError):
        bwd(m, 0, c, 40)
    with pytest.raises(L.MgarError):
        bwd(m, ns, c, c - 1)
    for name in ("mgar_voxel_roi_pool_fwd", "mgar_voxel_roi_pool_fwd_bf16"):
        for bad_ns in (0, 256):
            with pytest.raises(L.MgarError):
                fwd(name, m, bad_ns, c, 40)
        with pytest.raises(L.MgarError):
            fwd(name, m, ns, c, c - 1)
    # M = 0: OK, and nothing is written
    assert stats(0, ns, c) == 0 and bwd(0, ns, c, 40) == 0
    assert fwd("mgar_voxel_roi_pool_fwd", 0, ns, c, 40) == 0 and fwd("mgar_voxel_roi_pool_fwd_bf16", 0, ns, c, 40) == 0
    torch.cuda.synchronize()
    for t in (mean, invstd, moments, rm, rv, nbt, pooled, arg, dfeats, dgamma, dbeta, dw):
        assert (t == 5).all()


def test_workspace_sizes_are_the_documented_ones():
    """include/mgar_ops.h: stats 9 doubles per workgroup of the moments pass, min(2048, max(1, ceil(M nsample / 2048)));
    bwd ceil(M / 64) * C * 5 floats; MGAR_EINVAL (-1) for a negative argument."""
    L, _ = _mods()
    sw = lambda m, ns: L.raw("mgar_voxel_roi_pool_stats_workspace_doubles", m, ns)   # noqa: E731
    bw = lambda m, c: L.raw("mgar_voxel_roi_pool_bwd_workspace_floats", m, c)        # noqa: E731
    for m, ns in [(0, 8), (1, 1), (128, 16), (129, 16), (2117, 16), (70000, 16), (262144, 16), (270000, 16), (2000000, 255)]:
        assert sw(m, ns) == 9 * min(2048, max(1, -(-(m * ns) // 2048))), (m, ns)
    for m, c in [(0, 4), (1, 1), (64, 32), (65, 32), (2117, 32), (70000, 16)]:
        assert bw(m, c) == -(-m // 64) * c * 5, (m, c)
    assert sw(-1, 8) == -1 and sw(8, -1) == -1 and bw(-1, 4) == -1 and bw(4, -1) == -1
