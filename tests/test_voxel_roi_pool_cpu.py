"""Voxel-RoI pooling (csrc/voxel_roi_pool.hip) -- what can be pinned without a GPU.

The device test (tests/test_voxel_roi_pool_gpu.py) compares the kernels with `torch_refs.voxel_roi_pool_ref`, a float64
restatement of the reference's op chain (voxel_pool_modules.py:86-126), and with the closed forms the kernels use in place
of that chain.  Here, with no kernel involved:

* the closed forms are algebra, not approximation: w . E[r] and w^T Cov(r) w equal the chain's MEASURED BatchNorm mean and
  biased variance, and the d w_pos / d gamma / d beta expressions in the header comment of `vrp_bwd_finalize_kernel`
  equal autograd of the chain, to 1e-10, for batch statistics and for eval-mode (constant) statistics;
* the restated chain is the reference's: inside a float64 evaluation of NeighborVoxelSAModuleMSG it reproduces the
  reference project's own outputs, gradients and BatchNorm buffers (tests/golden/reference_pcdet_modules.npz);
* the conditions the device test relies on hold for its inputs (same generator, voxel_roi_pool_cases.py): at most 0.5 %
  of the non-empty (query, channel) entries are near-ties at margin 1e-5, and the one-sided conditioning case really has
  |E[r]| >= 5 std(r) on an axis."""
import pytest
import torch

import torch_refs as R
import voxel_roi_pool_cases as VC


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)


def _closed_form_grads(case, ref, w, gamma, train):
    """d gamma, d beta, d w_pos as vrp_bwd_kernel + vrp_bwd_finalize_kernel assemble them, in float64: only the arg-max
    neighbour of each (query, channel) carries gradient g = dpooled where pooled > 0;
        S0 = sum g,  S1 = sum g * phat,  S2 = sum g * r      (phat = (w_c . r - mean_c) * invstd_c)
        d beta = S0,  d gamma = S1,
        d w_c = gamma_c * invstd_c * (S2 - S0 * E[r] - S1 * invstd_c * Cov . w_c)      (eval: gamma_c * invstd_c * S2)."""
    w, gamma = w.detach(), gamma.detach()
    g = (torch.from_numpy(case["cot"]).double() * (ref.pooled.detach() > 0)).t()                  # (M, C)
    r = ref.r[torch.arange(ref.arg.shape[0])[:, None], ref.arg]                                   # (M, C, 3) of the arg-max
    invstd = 1.0 / torch.sqrt(ref.var.detach() + case["eps"])
    phat = ((r * w[None]).sum(-1) - ref.mean.detach()[None]) * invstd[None]                       # (M, C)
    s0, s1, s2 = g.sum(0), (g * phat).sum(0), (g[:, :, None] * r).sum(0)
    mo = ref.moments
    cov = torch.stack([mo[3], mo[4], mo[5], mo[4], mo[6], mo[7], mo[5], mo[7], mo[8]]).view(3, 3)
    d = s2
    if train:
        d = s2 - s0[:, None] * mo[:3][None] - (s1 * invstd)[:, None] * (w @ cov)
    return s1, s0, (gamma * invstd)[:, None] * d


@pytest.mark.parametrize("size", [(180, 16, 16), (2117, 16, 32), (4999, 8, 12), (333, 1, 1), (130, 255, 5), (5, 1, 3)], ids=VC.size_id)
@pytest.mark.parametrize("train", [True, False], ids=["train_stats", "eval_stats"])
def test_closed_forms_equal_the_measured_chain_in_float64(size, train):
    case = VC.make_case(*size)
    ref, feats, w, gamma, beta = VC.reference(case, train=train, requires_grad=True)
    if train:
        mo = ref.moments
        cov = torch.stack([mo[3], mo[4], mo[5], mo[4], mo[6], mo[7], mo[5], mo[7], mo[8]]).view(3, 3)
        wd = w.detach()
        assert mo[9].item() == size[0] * size[1]
        assert _rel(wd @ mo[:3], ref.mean.detach()) < 1e-10
        assert _rel(((wd @ cov) * wd).sum(1), ref.var.detach()) < 1e-10
    (ref.pooled * torch.from_numpy(case["cot"]).double()).sum().backward()
    dgamma, dbeta, dw = _closed_form_grads(case, ref, w, gamma, train)
    assert _rel(dgamma, gamma.grad) < 1e-10
    assert _rel(dbeta, beta.grad) < 1e-10
    assert _rel(dw, w.grad) < 1e-10, (_rel(dw, w.grad), dw, w.grad)


def test_reference_chain_reproduces_the_reference_projects_module():
    """NeighborVoxelSAModuleMSG in float64 with voxel_roi_pool_ref between mlps_in and mlps_out, integer decisions from the
    C oracle's voxel query, against the reference project's own module (the `voxel_sa_msg` fixture): output, input
    gradient, every parameter gradient and the BatchNorm buffers, at the 2e-5 of the oracle-backend test."""
    import numpy as np
    from oracle import oracle as O
    from test_reference_modules import CASES, _check, _cls, fill_deterministic, make_inputs
    case = next(c for c in CASES if c["name"] == "voxel_sa_msg")
    m = fill_deterministic(_cls(case)(**case["kwargs"]()), seed=case["seed"]).train().double()
    ins = make_inputs(case)
    args = [t.double().clone().requires_grad_(True) if rg else t for t, rg in ins]
    xyz, _, new_xyz, _, new_coords, features, v2p = args
    zyx = np.ascontiguousarray(new_coords[:, [0, 3, 2, 1]].numpy())
    outs = []
    for k, grouper in enumerate(m.groupers):
        feats_in = m.mlps_in[k](features.permute(1, 0).unsqueeze(0)).squeeze(0).permute(1, 0)
        idx_raw = O.voxel_query(grouper.max_range, grouper.radius, grouper.nsample, xyz.numpy(), new_xyz.numpy(), zyx, v2p.numpy())
        conv, bn = m.mlps_pos[k][0], m.mlps_pos[k][1]
        ref = R.voxel_roi_pool_ref(xyz, new_xyz, feats_in, torch.from_numpy(idx_raw), conv.weight.view(-1, 3), bn.weight, bn.bias,
                                   bn.eps, True, bn.running_mean, bn.running_var, bn.momentum)
        with torch.no_grad():
            bn.running_mean.copy_(ref.running_mean)
            bn.running_var.copy_(ref.running_var)
            bn.num_batches_tracked += 1
        outs.append(m.mlps_out[k](ref.pooled.unsqueeze(0)).squeeze(0).permute(1, 0))
    y = torch.cat(outs, 1)
    (y * torch.linspace(-1.0, 1.0, y.numel()).view(y.shape).double()).sum().backward()
    _check(case, m, args, ins, y, rtol=2e-5)


_TIE_CASES = [(s, None) for s in VC.FULL_SIZES] + [(VC.ALL_EMPTY, "all_empty")] + [(VC.CONDITIONING_SIZE, v) for v in VC.CONDITIONING]


@pytest.mark.parametrize("size,variant", _TIE_CASES, ids=["%s%s" % (VC.size_id(s), "_" + v if v else "") for s, v in _TIE_CASES])
def test_near_tie_share_of_the_device_cases_is_capped(size, variant):
    """A condition on the inputs, verified without the kernel: the device test exempts near-ties from its arg-max
    comparison and zeroes their cotangent, so they must be rare.  Measured: <= 1.3e-4 at every size."""
    case = VC.make_case(*size, variant=variant)
    ref = VC.reference(case)[0]
    idx = torch.from_numpy(case["idx_raw"])
    mask = R.near_tie_mask(ref.pre, idx, VC.NEAR_TIE_MARGIN)
    live = idx[:, 0] != -1
    assert not mask[~live].any()
    share = mask.sum().item() / max(live.sum().item() * size[2], 1)
    print("near-tie share %s %s: %.2e" % (VC.size_id(size), variant, share))
    assert share <= VC.NEAR_TIE_CAP


def test_near_tie_mask_ignores_padding_and_finds_a_planted_tie():
    idx = torch.tensor([[4, 9, 4, 4], [2, 3, 5, 6], [-1, 0, 0, 0]], dtype=torch.int32)
    v = torch.tensor([[[1.0, 0.2, 1.0, 1.0]], [[0.5, 2.0, 2.0 - 1e-7, 0.1]], [[0.3, 0.3, 0.3, 0.3]]], dtype=torch.float64)
    assert R.near_tie_mask(v, idx, 1e-5).tolist() == [[False], [True], [False]]
    assert R.near_tie_mask(v, idx, 1e-9).tolist() == [[False], [False], [False]]


def test_conditioning_cases_are_what_they_claim():
    ref = VC.reference(VC.make_case(*VC.CONDITIONING_SIZE, variant="one_sided"), stats_only=True)[0]
    r = ref.r.reshape(-1, 3)
    ratio = (r.mean(0).abs() / r.std(0, unbiased=False)).max().item()
    print("one-sided case: max_axis |E[r]| / std(r) = %.2f" % ratio)      # measured: 12.7
    assert ratio >= 5.0
    case = VC.make_case(*VC.CONDITIONING_SIZE, variant="translated")
    assert abs(case["xyz"][:, 0].mean() - 70.0) < 1.0 and abs(case["xyz"][:, 1].mean() + 40.0) < 1.0


def test_cap_case_is_beyond_the_block_cap_of_the_moments_pass():
    m, ns, _ = VC.CAP_CASE
    assert m * ns > 2048 * 256 * 8
