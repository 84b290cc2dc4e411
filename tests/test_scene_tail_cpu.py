"""CPU tests of the eval-mode fusion-net tail: the float64 reference of scene_tail_cases.py against the literal per-scene
formula of forward_per_scene, the margin conditions of both case families, and the plan's decisions (scene_tail_ops), all
without a device."""
import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_tail_cases as T


def test_cases_cover_what_they_promise():
    sizes = {n for c in T.CASES for n in c["counts"]}
    assert sizes >= set(T.SIZES)
    for fam in ("sep", "rnd"):
        cs = [c for c in T.CASES if c["family"] == fam]
        assert {c["D"] for c in cs} == {64, 512} and {c["mnp"] - max(c["counts"]) for c in cs} == {0, 1, 5}
        assert {c["hidden"] for c in cs} >= {0, 4} and all(len(c["counts"]) <= 6 and len(set(c["counts"])) > 1 for c in cs)


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_reference_is_the_literal_per_scene_formula(case):
    """The reference (dot / (|x_i| |x_j|), numpy) equals forward_per_scene's own lines in torch float64 (rows normalised first,
    then the product) to float64 rounding; ids and pooled rows agree on every row that keeps the margin."""
    ref, lit = T.reference(case), T.literal_per_scene(case)
    so, _, _ = SC.offsets(case["counts"])
    D = case["D"]
    for s, (n, (A, gid, pooled, card)) in enumerate(zip(case["counts"], lit)):
        assert np.abs(A.numpy() - ref["A"][s, :n, :n]).max() <= 1e-12
        assert (ref["A"][s, n:] == 0).all() and (ref["A"][s, :, n:] == 0).all() and (ref["gid"][s, n:] == -1).all()
        ok = ref["row_ok"][so[s]:so[s] + n]
        assert (gid.numpy()[ok] == ref["gid"][s, :n][ok]).all()
        assert (pooled.numpy()[ok] == ref["sg"][so[s]:so[s] + n][ok]).all()
        assert (card.numpy()[0, :D] == ref["colmax"][s]).all()
        assert abs(card.numpy()[0, D] - ref["card_sum"][s]) <= 1e-10 * n * n


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_margins(case):
    """sep: EVERY off-diagonal entry of the float64 adjacency is farther from 0.5 than 4 x its value bound; rnd: at least 90 %
    of the rows keep that margin on their whole row.  The bound itself stays far below the quantity it guards."""
    ref = T.reference(case)
    frac = float(ref["row_ok"].mean())
    print("scene_tail %s: rows keeping the margin %.4f, smallest clearance %.3g, largest value bound %.3g"
          % (T.case_id(case), frac, ref["min_clear"], ref["A_bound"].max()))
    assert ref["A_bound"].max() < 1e-3
    if case["family"] == "sep":
        assert ref["min_clear"] > 0 and frac == 1.0
        assert len({tuple(g) for g in ref["gid"]}) >= 1 and max(len(set(g[g >= 0])) for g in ref["gid"]) > 1   # several groups
    else:
        assert frac >= T.MIN_MARGIN_ROWS


def test_bound_bites():
    """A planted defect -- the dot product without its last term -- leaves the value bound by orders of magnitude."""
    case = T.CASES[0]
    ref, inp = T.reference(case), T.inputs(case)
    n = case["counts"][3]
    so, do, _ = SC.offsets(case["counts"])
    x = inp["x"][so[3]:so[3] + n].astype(np.float64)
    dg = inp["dg"][do[3]:do[3] + n * n].astype(np.float64).reshape(n, n)
    nrm = np.sqrt((x * x).sum(1))
    dv = (x[:, :-1] @ x[:, :-1].T) / (nrm[:, None] * nrm[None, :])
    a, _ = T.embed64(inp["params"], dv, dg, 0.0)
    np.fill_diagonal(a, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(a == ref["A"][3, :n, :n], 0.0, np.abs(a - ref["A"][3, :n, :n]) / ref["A_bound"][3, :n, :n])
    assert ratio.max() > 10.0


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _net(fusion="Attention_mat", modality="Multi", euclidean=True):
    from multimodal_gar_amd.model.gat_model import GAR_Fusion_Net3
    from multimodal_gar_amd.workload import model_cfg
    cfg = model_cfg(4, 256, fusion=fusion, modality=modality).GAR_MODEL
    cfg.EUCLIDEAN = euclidean
    return GAR_Fusion_Net3(cfg).eval().requires_grad_(False)


def test_plan_decisions_and_refusals(monkeypatch):
    """Every condition of the plan by itself, on the host: a tensor on the CPU that passes everything else is refused for its
    device alone, which is the last check."""
    from multimodal_gar_amd import scene_tail_ops as O
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    x = torch.zeros(8, 512)
    why = O.scene_tail_refusal
    for euclid, hidden in ((True, 0), (False, 4)):
        net = _net(euclidean=euclid)
        assert O._embed_parts(net.D_embed).hidden == hidden
        assert why(net, x, [4, 4]) == "device" and O.scene_tail_plan(net, x, [4, 4]) is None
    net = _net()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", False)
    assert why(net, x) == "switch off"
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    assert why(net.train(), x) == "training"
    net.eval()
    assert why(_net(fusion="crossAtt"), x) == "adjacency"
    assert why(_net(fusion="Attention"), x) == "adjacency" and why(_net(fusion="Attention_sum"), x) == "adjacency"
    for fusion in ("sum", "Attention_normal", "Attention_max", "Attention_multi", "Attention_gaussian", "catandAtt"):
        assert why(_net(fusion=fusion), x, [2, 128]) == "device"
    for modality in ("RGB", "LiDAR"):
        assert why(_net(modality=modality), x, [3, 5]) == "device"
    assert why(net, x, [1, 4]) == "configuration" and why(net, x, [129]) == "configuration"
    assert why(net, torch.zeros(8, 96), [4, 4]) == "size"
    assert why(net, x.double(), [4, 4]) == "payload" and why(net, x.view(2, 4, 512), [4, 4]) == "payload"
    with torch.enable_grad():
        assert why(net, x.clone().requires_grad_(True), [4, 4]) == "gradient"
        assert why(net, x, [4, 4]) == "device"                              # frozen parameters, plain input
        net.D_embed.requires_grad_(True)
        assert why(net, x, [4, 4]) == "gradient"
    with torch.no_grad():
        assert why(net, x, [4, 4]) == "device"                              # grad mode off: nothing needs one
    net.D_embed.requires_grad_(False)
    handle = net.D_embed.register_forward_hook(lambda *a: None)
    assert why(net, x, [4, 4]) == "hook"
    handle.remove()
    handle = net.D_embed[0].register_forward_pre_hook(lambda *a: None)
    assert why(net, x, [4, 4]) == "hook"
    handle.remove()
    net.D_embed = torch.nn.Sequential(torch.nn.Linear(2, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1), torch.nn.Sigmoid())
    assert why(net, x, [4, 4]) == "structure"                                # hidden width above 8


def test_parameter_block_layout_and_cache():
    from multimodal_gar_amd import scene_tail_ops as O
    for case in (T.CASES[0], T.CASES[1], T.CASES[4]):
        p = T.inputs(case)["params"]
        m = T.make_d_embed(p)
        block = O.embed_params(m)
        assert np.array_equal(block.numpy(), T.param_block(p))
        assert O.embed_params(m) is block                                   # cached
        with torch.no_grad():
            m[0].bias.add_(1.0)
        again = O.embed_params(m)                                           # an in-place update rebuilds
        assert again is not block and not np.array_equal(again.numpy(), T.param_block(p))


def test_eval_caches_keep_the_bits():
    """The cached stacked head parameters and the cached BatchNorm square root give the bits of the uncached expressions, and
    follow an in-place update of what they were built from."""
    from multimodal_gar_amd.model import gat_model as G
    torch.manual_seed(0)
    net = _net()
    bn = net.bn_rgb
    with torch.no_grad():
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0); bn.weight.normal_(); bn.bias.normal_()
        x = torch.randn(7, 512)
        for _ in range(2):
            want = (x - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps) * bn.weight + bn.bias
            assert torch.equal(G._eval_bn(bn, x), want) and torch.equal(G._eval_bn(bn, x), want)
            bn.running_var.mul_(1.5)
        feat = torch.randn(2 * 4, 1024)
        off = net._heads_stacked("", feat, 2, 4, 5)
        assert "_mgar_stacked_heads" in net.__dict__
        first = net.__dict__["_mgar_stacked_heads"][""][1]
        net._heads_stacked("", feat, 2, 4, 5)
        assert net.__dict__["_mgar_stacked_heads"][""][1] is first
    with torch.enable_grad():                                               # grad mode on: the uncached expressions
        on = net._heads_stacked("", feat, 2, 4, 5)
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    with torch.no_grad():
        getattr(net, G._HEAD_SPECS[0][0])[3].bias.add_(1.0)
        moved = net._heads_stacked("", feat, 2, 4, 5)
    assert net.__dict__["_mgar_stacked_heads"][""][1] is not first and not torch.equal(moved[0], off[0])
