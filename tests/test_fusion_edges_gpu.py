"""Fusion-head kernels (csrc/gatv2.hip, csrc/dafm.hip, csrc/roi_align.hip) at the shapes and edges the model reaches and
tests/test_fusion_ops_gpu.py does not: values and every gradient against the float64 references of torch_refs.py, at the
inputs of fusion_cases.py (tests/test_fusion_ops_cpu.py shows those references right and those inputs clear of RoIAlign's
discontinuities).  Tolerance as in test_fusion_ops_gpu.py: 1e-4 relative to the largest reference value + 1e-5
(BASELINE.json north_star); parameter gradients -- sums over all edges with heavy cancellation -- may instead stay within
3x the error of a plain fp32 torch evaluation of the same reference."""
import functools

import pytest
import torch

import fusion_cases as FC
import torch_refs as R

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
BF = torch.bfloat16


def close(a, b, what=""):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item() + 1e-12 if b.numel() else 0.0
    err = (a - b).abs().max().item() if b.numel() else 0.0
    print("%s: err %.3e scale %.3e" % (what, err, scale))
    assert err <= ATOL + RTOL * scale, "%s: max err %g vs scale %g" % (what, err, scale)


# ------------------------------------------------------------------------------------------------ GATv2
def _gat_modules(case):
    """The device module, its float64 CPU twin and its fp32 device twin (for the plain-torch fp32 yardstick)."""
    from multimodal_gar_amd.graph_ops import GATv2Conv
    opts = dict(concat=case.get("concat", False), add_self_loops=case.get("add_self_loops", True), bias=case.get("bias", True),
                share_weights=case.get("share_weights", False))
    H, C = case["H"], case["C"]
    torch.manual_seed(2)
    conv = GATv2Conv(C, C, H, dropout=0.5, **opts).cuda()
    with torch.no_grad():                               # non-zero biases, so that a dropped bias shows
        for p in (conv.lin_l.bias, conv.lin_r.bias, conv.bias):
            if p is not None:
                p.uniform_(-0.5, 0.5)
    ref = GATv2Conv(C, C, H, dropout=0.5, **opts).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in conv.state_dict().items()})
    c32 = GATv2Conv(C, C, H, dropout=0.5, **opts).cuda()
    c32.load_state_dict(conv.state_dict())
    return conv, ref, c32, opts


def _gat_check(case):
    n, H, C, train = case["n"], case["H"], case["C"], case.get("train", False)
    conv, ref_conv, conv32, opts = _gat_modules(case)
    conv.train(train)
    x = (torch.randn(n, C) * case.get("x_scale", 1.0)).cuda().requires_grad_(True)
    edge_index = FC.gat_graph(case["graph"], n).cuda()
    torch.manual_seed(7)
    out, (rowptr, col, alpha) = conv(x, edge_index, return_attention_weights=True)
    assert not alpha.requires_grad
    g = torch.randn_like(out)
    out.backward(g)
    rp, cl = rowptr.cpu().tolist(), col.cpu().tolist()
    edge_scale = None
    if train:  # replay the same dropout mask in the reference
        torch.manual_seed(7)
        mask = torch.bernoulli(torch.full((col.numel(), H), 0.5, device="cuda")) / 0.5
        edge_scale = {(cl[e], i): mask[e].double().cpu() for i in range(n) for e in range(rp[i], rp[i + 1])}
        assert len(edge_scale) == col.numel()           # no duplicates: the dict is faithful
    kw = dict(concat=opts["concat"], add_self_loops=opts["add_self_loops"], share_weights=opts["share_weights"])
    xd = x.detach().double().cpu().requires_grad_(True)
    ref, ref_alpha = R.gatv2_ref(xd, edge_index.cpu(), ref_conv.lin_l, ref_conv.lin_r, ref_conv.att, ref_conv.bias, H, C,
                                 edge_scale=edge_scale, return_alpha=True, **kw)
    ref.backward(g.double().cpu())
    close(out, ref, "out")
    close(alpha, ref_alpha, "alpha")
    sums = torch.stack([alpha[rp[i]:rp[i + 1]].sum(0) for i in range(n) if rp[i + 1] > rp[i]])
    assert (sums - 1).abs().max().item() <= 1e-5, (sums - 1).abs().max().item()
    close(x.grad, xd.grad, "x.grad")
    x32 = x.detach().clone().requires_grad_(True)
    es32 = None if edge_scale is None else {k_: v_.float().cuda() for k_, v_ in edge_scale.items()}
    ref32 = R.gatv2_ref(x32, edge_index.cpu(), conv32.lin_l, conv32.lin_r, conv32.att, conv32.bias, H, C, edge_scale=es32, **kw)
    ref32.backward(g)
    names = [na for na, _ in conv.named_parameters()]
    assert names == [nb for nb, _ in ref_conv.named_parameters()] == [nc for nc, _ in conv32.named_parameters()]
    assert ("bias" in names) == opts["bias"] and ("lin_r.weight" in names) == (not opts["share_weights"])
    for na, pa, pb, pc in zip(names, conv.parameters(), ref_conv.parameters(), conv32.parameters()):
        scale = pb.grad.abs().max().item() + 1e-12
        err = (pa.grad.double().cpu() - pb.grad).abs().max().item()
        err32 = (pc.grad.double().cpu() - pb.grad).abs().max().item()
        print("%s.grad: err %.3e torch-fp32 err %.3e scale %.3e" % (na, err, err32, scale))
        assert err <= max(ATOL + RTOL * scale, 3.0 * err32), "%s: err %g, torch-fp32 err %g, scale %g" % (na, err, err32, scale)
    # no float atomics in the backward: every sum has a fixed order, a second run gives the same bits
    first = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    x.grad = None
    conv.zero_grad(set_to_none=True)
    torch.manual_seed(7)
    out2 = conv(x, edge_index)
    out2.backward(g)
    assert torch.equal(out, out2)
    for a, b in zip(first, [x.grad] + [p.grad for p in conv.parameters()]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(FC.GAT_CASES))
def test_gatv2_case(name):
    _gat_check(FC.GAT_CASES[name])


def test_gatv2_saturated_softmax():
    """x scaled by 30: the logits reach into the hundreds; the running max keeps __expf in range."""
    _gat_check(FC.GAT_SATURATED)


def test_gatv2_aggregate_without_self_loops_empty_ranges():
    """add_self_loops=False, straight on the Function: a target without incoming edge (e0 == e1, emax = -inf, inv = 0)
    aggregates exactly 0 and sends exactly 0 to x_r; a source without outgoing edge gets exactly 0 for x_l."""
    from multimodal_gar_amd.graph_ops import _GatAggregate, edges_to_csr
    n, H, C = 12, 2, 64
    torch.manual_seed(3)
    rowptr, col = edges_to_csr(FC.holes_graph(n).cuda(), n, add_self_loops=False)
    xl = torch.randn(n, H * C, device="cuda", requires_grad=True)
    xr = torch.randn(n, H * C, device="cuda", requires_grad=True)
    att = torch.randn(H, C, device="cuda", requires_grad=True)
    out, alpha = _GatAggregate.apply(xl, xr, att, rowptr, col, None, H, 0.2)
    out.backward(torch.randn_like(out))
    assert torch.isfinite(out).all() and torch.isfinite(alpha).all()
    for g in (xl.grad, xr.grad, att.grad):
        assert torch.isfinite(g).all()
    rp = rowptr.cpu().tolist()
    for i in range(n):
        empty = i in FC.HOLES_NO_INCOMING
        assert (rp[i + 1] == rp[i]) == empty
        assert bool((out[i] == 0).all()) == empty
        if empty:
            assert (xr.grad[i] == 0).all()
        elif rp[i + 1] - rp[i] >= 2:                    # one incoming edge: alpha = 1, de = 0, nothing reaches x_r either
            assert (xr.grad[i] != 0).any()
        assert bool((xl.grad[i] == 0).all()) == (i in FC.HOLES_NO_OUTGOING)


def test_gatv2_csr_cache_follows_in_place_edits():
    """The CSR form is cached on the edge tensor, keyed by its _version: an in-place edit must rebuild it."""
    from multimodal_gar_amd.graph_ops import GATv2Conv
    torch.manual_seed(4)
    n, H, C = 10, 2, 64
    conv = GATv2Conv(C, C, H, concat=False).cuda().eval()
    x = torch.randn(n, C, device="cuda")
    ei = FC.random_graph(n, 30, 5, loops=False)
    same_target = [(a, b) for a in range(ei.shape[1]) for b in range(a + 1, ei.shape[1])
                   if ei[1, a] == ei[1, b] and ei[0, a] != ei[0, b]]
    a, b = same_target[0]
    ei = ei.cuda()
    with torch.no_grad():
        out0, (_, col0, alpha0) = conv(x, ei, return_attention_weights=True)
        assert hasattr(ei, "_mgar_csr")
        out0b, (_, col0b, _) = conv(x, ei, return_attention_weights=True)
        assert col0b is col0 and torch.equal(out0, out0b)                  # the cache is used
        ei[:, [a, b]] = ei[:, [b, a]]                                      # same graph, other edge order within a target
        out1, (_, col1, alpha1) = conv(x, ei, return_attention_weights=True)
        fresh = ei.clone()
        out1f, (_, col1f, alpha1f) = conv(x, fresh, return_attention_weights=True)
        assert not torch.equal(col1, col0)                                 # a stale CSR would show
        assert torch.equal(col1, col1f) and torch.equal(alpha1, alpha1f) and torch.equal(out1, out1f)
        old_target = int(ei[1, a])
        ei[1, a] = (old_target + 1) % n if (old_target + 1) % n != int(ei[0, a]) else (old_target + 2) % n   # another graph
        out2, (rp2, col2, alpha2) = conv(x, ei, return_attention_weights=True)
        out2f, (rp2f, col2f, alpha2f) = conv(x, ei.clone(), return_attention_weights=True)
        assert torch.equal(rp2, rp2f) and torch.equal(col2, col2f) and torch.equal(alpha2, alpha2f) and torch.equal(out2, out2f)
        assert not torch.equal(out2, out1)


def test_gatv2_alpha_is_not_differentiable_and_out_gradients_are_unchanged():
    from multimodal_gar_amd.graph_ops import _GatAggregate, edges_to_csr
    n, H, C = 7, 2, 64
    torch.manual_seed(5)
    rowptr, col = edges_to_csr(FC.complete_graph(n).cuda(), n)
    leaves = [torch.randn(n, H * C, device="cuda"), torch.randn(n, H * C, device="cuda"), torch.randn(H, C, device="cuda")]
    g = torch.randn(n, H * C, device="cuda")
    grads = []
    for touch_alpha in (False, True):
        xl, xr, att = (t.clone().requires_grad_(True) for t in leaves)
        out, alpha = _GatAggregate.apply(xl, xr, att, rowptr, col, None, H, 0.2)
        assert out.requires_grad and not alpha.requires_grad
        loss = (out * g).sum() + (alpha.sum() * 3.0 if touch_alpha else 0.0)    # alpha is a constant of the graph
        loss.backward()
        grads.append((xl.grad, xr.grad, att.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ DAFM
@pytest.mark.parametrize("name", list(FC.DAFM_CASES))
def test_dafm_case(name):
    from multimodal_gar_amd.dafm_ops import dafm_attention, scene_offsets
    case = FC.DAFM_CASES[name]
    counts, D = case["counts"], case["D"]
    q0, k0, v0, des, g = FC.dafm_inputs(counts, D, case.get("de_max", 20.0), case.get("qk_scale", 1.0))
    q, k, v = (t.cuda().requires_grad_(True) for t in (q0, k0, v0))
    de_flat = torch.cat([d.reshape(-1) for d in des]).cuda()
    so, do = scene_offsets(counts, "cuda")
    scale = 1.0 / D ** 0.5
    out, att = dafm_attention(q, k, v, de_flat, so, do, FC.DAFM_SIGMA, scale)
    assert out.requires_grad and not att.requires_grad
    assert att.shape == de_flat.shape
    out.backward(g.cuda())
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q0, k0, v0))
    r0, refs, ref_att = 0, [], []
    for n, d in zip(counts, des):
        if n:
            o, a = R.dafm_ref(qd[r0:r0 + n], kd[r0:r0 + n], vd[r0:r0 + n], d.double(), FC.DAFM_SIGMA, scale)
            refs.append(o); ref_att.append(a.detach().reshape(-1))
        r0 += n
    ref = torch.cat(refs)
    ref.backward(g.double())
    close(out, ref, "out")
    close(att, torch.cat(ref_att), "att")
    m0 = 0
    for n in counts:                                    # every row of every scene's att sums to 1
        if n:
            rows = att[m0:m0 + n * n].view(n, n).sum(1)
            assert (rows - 1).abs().max().item() <= 1e-5, (n, (rows - 1).abs().max().item())
        m0 += n * n
    close(q.grad, qd.grad, "dq"); close(k.grad, kd.grad, "dk"); close(v.grad, vd.grad, "dv")


def test_dafm_scene_above_capacity_raises_before_any_launch():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import scene_offsets
    from multimodal_gar_amd.model.gat_model import FusionAttention_mat
    with pytest.raises(ValueError, match="MGAR_DAFM_MAX_N"):
        scene_offsets([5, L.DAFM_MAX_N + 1], "cuda")
    n = L.DAFM_MAX_N + 1
    mod = FusionAttention_mat(64, 64).cuda()
    launched = []
    real = L.call
    try:
        L.call = lambda name, *a: (launched.append(name), real(name, *a))[1]
        with pytest.raises(ValueError, match="MGAR_DAFM_MAX_N"):
            mod(torch.randn(n, 64, device="cuda"), torch.randn(n, 64, device="cuda"), None, torch.rand(n, n, device="cuda"))
    finally:
        L.call = real
    assert launched == []


def test_dafm_att_is_not_differentiable_and_out_gradients_are_unchanged():
    from multimodal_gar_amd.dafm_ops import dafm_attention, scene_offsets
    counts, D = [6, 3], 64
    q0, k0, v0, des, g = FC.dafm_inputs(counts, D, seed=6)
    de_flat = torch.cat([d.reshape(-1) for d in des]).cuda()
    so, do = scene_offsets(counts, "cuda")
    grads = []
    for touch_att in (False, True):
        q, k, v = (t.cuda().requires_grad_(True) for t in (q0, k0, v0))
        out, att = dafm_attention(q, k, v, de_flat, so, do, FC.DAFM_SIGMA, 0.125)
        assert out.requires_grad and not att.requires_grad
        loss = (out * g.cuda()).sum() + (att.sum() * 3.0 if touch_att else 0.0)
        loss.backward()
        grads.append((q.grad, k.grad, v.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ RoIAlign
@functools.lru_cache(maxsize=None)
def _roi_reference(name):
    """(case, float64 output, float64 input gradient, upstream gradient) -- computed once per case, never modified."""
    c = FC.ROI_CASES[name]()
    f = torch.from_numpy(c["feat"]).double().requires_grad_(True)
    ref = R.roi_align_ref(f, torch.from_numpy(c["rois"]), c["out_size"], c["scale"], c["sampling_ratio"], c["aligned"])
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64).float()
    ref.backward(g.double())
    return c, ref.detach(), f.grad, g


@pytest.mark.parametrize("name", list(FC.ROI_CASES))
def test_roi_align_case(name):
    from multimodal_gar_amd.vision_ops import roi_align
    c, ref, ref_grad, g = _roi_reference(name)
    f = torch.from_numpy(c["feat"]).cuda().requires_grad_(True)
    rois = torch.from_numpy(c["rois"]).cuda()
    out = roi_align(f, rois, c["out_size"], c["scale"], c["sampling_ratio"], c["aligned"])
    ph, pw = (c["out_size"],) * 2 if isinstance(c["out_size"], int) else c["out_size"]
    assert out.shape == (len(c["rois"]), c["feat"].shape[1], ph, pw)
    out.backward(g.cuda())
    close(out, ref, "out")
    close(f.grad, ref_grad, "input grad")
    if name == "degenerate_aligned":                    # no counted sample: exactly 0
        assert (out[list(FC.ROI_DEGENERATE_ZERO_OUTPUT)] == 0).all()


def test_roi_align_grid_stride_bf16_equals_rounded_fp32():
    """The bf16 twin beyond the launch cap, by the rule of test_bf16_gpu.py: it computes in fp32 and rounds once on store,
    so on bf16-representable inputs its result EQUALS the fp32 kernel's result rounded to bf16."""
    from multimodal_gar_amd.vision_ops import roi_align
    c, ref, _, _ = _roi_reference("grid_stride")
    fm = torch.from_numpy(c["feat"]).to(BF).float().cuda()
    rois = torch.from_numpy(c["rois"]).cuda()
    with torch.no_grad():
        a = roi_align(fm, rois, c["out_size"], c["scale"])
        b = roi_align(fm.to(BF), rois, c["out_size"], c["scale"])
    assert a.numel() > 16384 * 256
    assert b.dtype == BF and torch.equal(b, a.to(BF))
    tail = a.reshape(-1)[16384 * 256:]                  # the outputs only the second grid-stride trip writes
    assert tail.abs().max().item() > 0.1
