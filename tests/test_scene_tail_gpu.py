"""Device tests of the eval-mode fusion-net tail: the kernel (mgar_scene_tail_eval_fwd, csrc/scene_tail_eval.hip) against the
float64 reference and per-element bounds of scene_tail_cases.py, bit repeatability, scene independence, NaN containment, exact
padding and refusals; GAR_Fusion_Net3's routing (scene_tail_ops.scene_tail_plan), switch on against switch off, the reference's
own eval outputs with the switch on, and graph capture."""
import os

import numpy as np
import pytest
import torch

import scene_cases as SC
import scene_tail_cases as T
import test_fusion_variants_gpu as V

pytestmark = pytest.mark.gpu
ENTRY = "mgar_scene_tail_eval_fwd"


def _mods():
    from multimodal_gar_amd import _lib, scene_tail_ops
    return _lib, scene_tail_ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _launch(counts, mnp, x, dg, block, hidden):
    """host arrays -> the four device outputs of the entry point"""
    _, O = _mods()
    so, do, _ = SC.offsets(counts)
    so_d, do_d = _dev(so, torch.int32), _dev(do, torch.int32)
    out = O.scene_tail_eval_fwd(_dev(x), _dev(dg), so_d, do_d, counts, mnp, _dev(block), hidden)
    torch.cuda.synchronize()
    return out


def _launch_case(case, x=None):
    inp = T.inputs(case)
    return _launch(case["counts"], case["mnp"], inp["x"] if x is None else x, inp["dg"], T.param_block(inp["params"]),
                   case["hidden"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_values_ids_and_pooled_rows(case):
    """A_list and the card sum inside their bounds everywhere (padding exactly 0 / -1); the column maxima exact; group ids and
    pooled rows exact on every row whose reference adjacency row keeps the margin -- all rows of the separable family.
    Measured max err / bound on an MI355X: see DESIGN.md section 3.13g."""
    ref = T.reference(case)
    A, gid, sg, card = (t.cpu().numpy() for t in _launch_case(case))
    D, counts = case["D"], case["counts"]
    so, _, _ = SC.offsets(counts)
    r_a = _ratio(np.abs(A.astype(np.float64) - ref["A"]), ref["A_bound"])
    r_c = _ratio(np.abs(card[:, D].astype(np.float64) - ref["card_sum"]), ref["card_sum_bound"])
    print("scene_tail %s: max err / bound A_list %.3g, card sum %.3g" % (T.case_id(case), r_a, r_c))
    assert np.isfinite(A).all() and r_a <= 1.0 and r_c <= 1.0
    assert (card[:, :D].astype(np.float64) == ref["colmax"]).all()
    for s, n in enumerate(counts):
        assert (A[s, n:] == 0).all() and (A[s, :, n:] == 0).all() and (gid[s, n:] == -1).all()
        assert (np.diagonal(A[s, :n, :n]) == 1).all()
    ok = ref["row_ok"]
    got_gid = np.concatenate([gid[s, :n] for s, n in enumerate(counts)])
    want_gid = np.concatenate([ref["gid"][s, :n] for s, n in enumerate(counts)])
    if case["family"] == "sep":
        assert ok.all()
    assert ok.mean() >= T.MIN_MARGIN_ROWS
    assert (got_gid[ok] == want_gid[ok]).all()
    # a pooled row depends on the ids of all rows of its scene: compared where the whole scene's ids agree, else row by row
    # on the rows whose group has the reference's members
    same = got_gid == want_gid
    for s, n in enumerate(counts):
        rows = slice(so[s], so[s] + n)
        if same[rows].all():
            assert (sg[rows].astype(np.float64) == ref["sg"][rows]).all()
        else:
            assert case["family"] == "rnd"
            g = got_gid[rows]
            x = T.inputs(case)["x"][rows].astype(np.float64)
            for i in range(n):                              # the kernel's own ids, pooled in float64: still an exact check
                assert (sg[so[s] + i].astype(np.float64) == x[g == g[i]].max(0)).all()


@pytest.mark.parametrize("case", [T.CASES[1], T.CASES[10]], ids=T.case_id)
def test_bit_repeatable_and_scene_independent(case):
    """The same launch twice gives the same bits; every scene launched alone -- another S, other offsets, another mnp, no
    neighbours -- gives the bits it has among the others."""
    inp = T.inputs(case)
    a, b = _launch_case(case), _launch_case(case)
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))
    so, do, _ = SC.offsets(case["counts"])
    block = T.param_block(inp["params"])
    for s, n in enumerate(case["counts"]):
        A, gid, sg, card = _launch([n], n, inp["x"][so[s]:so[s] + n], inp["dg"][do[s]:do[s] + n * n], block, case["hidden"])
        assert torch.equal(_bits(A[0]), _bits(a[0][s, :n, :n])) and torch.equal(gid[0], a[1][s, :n])
        assert torch.equal(_bits(sg), _bits(a[2][so[s]:so[s] + n])) and torch.equal(_bits(card[0]), _bits(a[3][s]))


@pytest.mark.parametrize("kind", ["nan", "zero_row"])
@pytest.mark.parametrize("case", [T.CASES[0], T.CASES[9]], ids=T.case_id)
def test_nan_stays_in_its_scene(case, kind):
    """One NaN element, or one all-zero row (norm 0, so 0 / 0), in one scene: every other scene keeps the bits of the clean
    run.  In the hit scene the row and the column of the bad actor are NaN off the diagonal, the diagonal is still 1, the
    actor's id is its own index (a NaN compares false), its group's pooled row and the column maximum carry the NaN (the
    zero row carries none), and the card sum is NaN."""
    inp = T.inputs(case)
    clean = _launch_case(case)
    hit = 2
    so, _, _ = SC.offsets(case["counts"])
    n, D = case["counts"][hit], case["D"]
    bad_i = n // 2
    x = inp["x"].copy()
    if kind == "nan":
        x[so[hit] + bad_i, 5] = np.nan
    else:
        x[so[hit] + bad_i] = 0.0
    A, gid, sg, card = _launch_case(case, x)
    for s in range(len(case["counts"])):
        if s == hit:
            continue
        rows = slice(so[s], so[s + 1])
        assert torch.equal(_bits(A[s]), _bits(clean[0][s])) and torch.equal(gid[s], clean[1][s])
        assert torch.equal(_bits(sg[rows]), _bits(clean[2][rows])) and torch.equal(_bits(card[s]), _bits(clean[3][s]))
    Ah = A[hit, :n, :n].cpu().numpy()
    off = ~np.eye(n, dtype=bool)
    assert np.isnan(Ah[bad_i][off[bad_i]]).all() and np.isnan(Ah[:, bad_i][off[:, bad_i]]).all()
    assert (np.diagonal(Ah) == 1).all() and int(gid[hit, bad_i]) == bad_i
    clean_rows = np.delete(np.arange(n), bad_i)
    assert np.isfinite(Ah[np.ix_(clean_rows, clean_rows)]).all()
    assert bool(torch.isnan(card[hit, D]))
    g = gid[hit, :n].cpu().numpy()
    sgh, cm = sg[so[hit]:so[hit] + n].cpu().numpy(), card[hit, :D].cpu().numpy()
    members = g == g[bad_i]
    if kind == "nan":
        assert np.isnan(sgh[members, 5]).all() and np.isfinite(np.delete(sgh, 5, axis=1)).all()
        assert np.isfinite(sgh[~members]).all() and np.isnan(cm[5]) and np.isfinite(np.delete(cm, 5)).all()
    else:
        assert np.isfinite(sgh).all() and np.isfinite(cm).all()
    assert (A[hit, n:] == 0).all() and (A[hit, :, n:] == 0).all() and (gid[hit, n:] == -1).all()


def test_refusals():
    """Scene sizes outside 2..128, a scene wider than mnp, D % 64 != 0 and hidden > 8 return MGAR_EUNSUPPORTED, bad sizes and
    null pointers MGAR_EINVAL, S == 0 MGAR_OK -- all before any launch: the outputs keep their bits; the host wrapper raises."""
    L, O = _mods()
    f = L._fns[ENTRY]
    D, mnp = 64, 6
    x, dg = torch.randn(8, D, device="cuda"), torch.randn(32, device="cuda")
    so, do = _dev(np.array([0, 4, 8]), torch.int32), _dev(np.array([0, 16]), torch.int32)
    par = torch.zeros(33, device="cuda")
    A = torch.full((2, mnp, mnp), -7.0, device="cuda"); gid = torch.full((2, mnp), -7, dtype=torch.int32, device="cuda")
    sg = torch.full((8, D), -7.0, device="cuda"); card = torch.full((2, D + 1), -7.0, device="cuda")
    st = L.stream_of(x)
    outs = (A.data_ptr(), gid.data_ptr(), sg.data_ptr(), card.data_ptr())

    def call(S=2, rows=8, d=D, m=mnp, lo=4, hi=4, hidden=0, xp=x.data_ptr(), o=outs):
        return f(S, rows, d, m, lo, hi, so.data_ptr(), do.data_ptr(), xp, dg.data_ptr(), par.data_ptr(), hidden, *o, st)
    assert call(lo=1) == -3 and call(hi=129, m=200) == -3 and call(hi=7) == -3          # n = 1, n = 129, n > mnp
    assert call(d=96) == -3 and call(d=32) == -3 and call(hidden=9) == -3
    assert call(S=-1) == -1 and call(d=0) == -1 and call(m=0) == -1 and call(hidden=-1) == -1
    assert call(xp=None) == -1 and call(o=(None,) + outs[1:]) == -1 and call(o=outs[:1] + (None,) + outs[2:]) == -1
    assert call(S=0, rows=0, lo=0, hi=0, xp=None, o=(None,) * 4) == 0
    assert b"scene" in L._fns["mgar_last_error"]()
    torch.cuda.synchronize()
    assert (A == -7).all() and (gid == -7).all() and (sg == -7).all() and (card == -7).all()
    for counts, m, d in (([4, 1], 6, 64), ([4, 7], 6, 64), ([4, 4], 6, 96)):
        rows, pairs = sum(counts), sum(c * c for c in counts)
        so2, do2, _ = SC.offsets(counts)
        with pytest.raises(L.MgarError):
            O.scene_tail_eval_fwd(torch.randn(rows, d, device="cuda"), torch.randn(pairs, device="cuda"), _dev(so2, torch.int32),
                                  _dev(do2, torch.int32), counts, m, par[:3].clone(), 0)
    with pytest.raises(L.MgarError):
        O.scene_tail_eval_fwd(torch.randn(8, 64), torch.randn(32), so.cpu(), do.cpu(), [4, 4], 6, par[:3].cpu(), 0)


# ---- the fusion net -----------------------------------------------------------------------------------------------------------------
class _Calls:
    """Counts the calls of the library's entry points made while it is active."""

    def __enter__(self):
        L, _ = _mods()
        self.L, self.real, self.n = L, dict(L._fns), {}
        for name, fn in self.real.items():
            L._fns[name] = (lambda name, fn: lambda *a: (self.n.__setitem__(name, self.n.get(name, 0) + 1), fn(*a))[1])(name, fn)
        return self.n

    def __exit__(self, *exc):
        self.L._fns.update(self.real)


def _forward(net, batch):
    rgb, lid, bb, b3, pid = batch
    return net(rgb, lid, bb, b3, None, pid)


def test_routing(monkeypatch):
    """Eval mode without a required gradient takes the kernel, once, on _forward_batched and on forward_packed, under both
    D_embed forms and for one modality; train mode, a required gradient, crossAtt and the switch off keep the old route, whose
    eval outputs the switch does not touch."""
    _, O = _mods()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    uniform, ragged = V._batch((5, 5, 5), 21), V._batch((2, 7, 33, 5, 12), 21)

    def calls(net, batch, grad=False):
        with torch.set_grad_enabled(grad), _Calls() as n:
            _forward(net, batch)
        return n.get(ENTRY, 0), n.get("mgar_scene_gram_fwd", 0)
    frozen = lambda *a, **k: V._net(*a, **k).requires_grad_(False)                                 # noqa: E731
    assert V._routes_called(V._net("Attention_mat", False), uniform) == ["_forward_batched"]
    assert calls(V._net("Attention_mat", False), uniform) == (1, 0)
    assert calls(V._net("Attention_mat", False), ragged) == (1, 0)
    assert calls(V._net("Attention_mat", False, EUCLIDEAN=False), ragged) == (1, 0)
    assert calls(V._net("sum", False), ragged) == (1, 0) and calls(V._net("catandAtt", False), ragged) == (1, 0)
    assert calls(V._net("Attention_mat", False, MODALITY="RGB", FEAT_NORM=False, FEATURE_DIM=512), ragged) == (1, 0)
    assert calls(frozen("Attention_mat", False), ragged, grad=True) == (1, 0)                       # nothing wants a gradient
    assert calls(V._net("Attention_mat", True), ragged) == (0, 1)                                   # train mode
    assert calls(V._net("Attention_mat", False), ragged, grad=True) == (0, 1)                       # parameters want one
    assert calls(V._net("crossAtt", False), ragged)[0] == 0
    assert calls(V._net("Attention_mat", False, DISABLE_BATCHED=True), ragged)[0] == 0              # scene by scene
    hooked = V._net("Attention_mat", False)
    hooked.D_embed.register_forward_hook(lambda *a: None)
    assert calls(hooked, ragged) == (0, 1)
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", False)
    assert calls(V._net("Attention_mat", False), ragged) == (0, 1) and calls(V._net("Attention_mat", False), uniform)[0] == 0


@pytest.mark.parametrize("euclidean", [True, False], ids=["linear", "hidden4"])
@pytest.mark.parametrize("counts", [(5, 5, 5), (2, 7, 33, 5, 12)], ids=["batched", "packed"])
def test_switch_on_against_switch_off(counts, euclidean, monkeypatch):
    """The same net and batch with the switch on and off: A_list and the card output agree within the value bound (D = 512, evaluated
    with |Dv| <= 1 and |Dg| <= 1 and the net's parameters), the individual
    heads are bit-equal, the group heads are bit-equal on every scene whose ids agree, and the kernel's ids are the ids of its
    own A_list.  Invalid if fewer than 90 % of the rows keep the margin on the switch-off output."""
    _, O = _mods()
    batch = V._batch(counts, 21)
    net = V._net("Attention_mat", False, EUCLIDEAN=euclidean)
    with torch.no_grad():
        monkeypatch.setattr(O, "SCENE_TAIL_FUSE", False)
        off = _forward(net, batch)
        monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
        on = _forward(net, batch)
        gid = net._tail_group_id
    from torch_refs import gamma_u as g
    bound = T.worst_case_value_bound(net.D_embed, 512)
    rows_ok = T.margin_rows(off[0].cpu().numpy(), counts, bound)
    frac = float(np.concatenate(rows_ok).mean())
    err = float((on[0].double() - off[0].double()).abs().max())
    print("scene_tail on/off %s %s: max |dA| %.3g, bound %.3g, rows keeping the margin %.3f" % (counts, euclidean, err, bound, frac))
    assert frac >= 0.9, "invalid: too few rows keep the margin on the switch-off output"
    assert err <= bound
    mnp = off[0].shape[1]
    for s, n in enumerate(counts):
        assert not on[0][s, n:].any() and not on[0][s, :, n:].any() and (gid[s, n:] == -1).all()
        want = net._predicted_groups(on[0][s, :n, :n])
        assert torch.equal(gid[s, :n].long(), want)
        same = torch.equal(want, net._predicted_groups(off[0][s, :n, :n]))
        assert same or not rows_ok[s].all()
        for i in range(1, 8):
            assert torch.equal(_bits(on[i][s]), _bits(off[i][s]))
        if same:
            for i in range(8, 15):
                assert torch.equal(_bits(on[i][s]), _bits(off[i][s])), (s, i)
    assert gid.shape == (len(counts), mnp) and gid.dtype == torch.int32
    # card_net is a Linear(513, 512) + ReLU + Linear(512, 1) on [column maxima (equal bits), block sum (within its bound)]
    card_err = float((on[15].double() - off[15].double()).abs().max())
    w = [t.detach().double() for t in net.card_net.parameters()]
    n_max = max(counts)
    sum_bound = n_max * n_max * bound + g(2 * n_max) * n_max * n_max
    lipschitz = float((w[2].abs() @ w[0][:, 512].abs()).max())
    scale = float(off[15].double().abs().max()) + 1.0
    assert card_err <= lipschitz * sum_bound + g(1030) * scale * float(w[2].abs().sum() + 1), card_err


HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("route", ["batched", "packed"])
def test_reference_golden_blocks_with_the_switch_on(route, monkeypatch):
    """tests/golden/reference_torch_blocks.npz: the reference net's eval outputs at test_reference_blocks.py's 2e-4, on the
    fused tail (asserted: one call of the entry point)."""
    _, O = _mods()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    G = V.BLOCKS
    net = V._net("Attention_mat", False)
    rgb, lid, bb, b3 = (torch.from_numpy(G[k]).cuda() for k in ("gar_rgb", "gar_lidar", "gar_bboxes", "gar_bboxes3d"))
    pid = torch.from_numpy(G["gar_pid"]).cuda()
    with torch.no_grad(), _Calls() as n:
        if route == "batched":
            res = net(rgb, lid, bb, b3, None, pid)
        else:
            counts = net._scene_counts(rgb, lid, pid)
            res = net._forward_ragged(rgb, lid, bb, b3, counts)
    assert n.get(ENTRY, 0) == 1 and len(res) == 16
    for i, r in enumerate(res):
        V.close(r, G["gar_eval_%02d" % i], rtol=2e-4)


def _table_params():
    import scene_mha_cases as MC
    return [(c, k) for c in MC.CONFIGS for k in MC.NET_COUNTS]


@pytest.mark.parametrize("config,counts", _table_params(), ids=lambda v: v if isinstance(v, str) else "".join(map(str, v)))
def test_reference_fusion_table_with_the_switch_on(config, counts, monkeypatch):
    """tests/golden/reference_fusion_table.npz, eval mode, packed route, at test_fusion_table_gpu.py's 2e-4: catandAtt and the
    single-modality baselines on the fused tail (one call), crossAtt on its own adjacency (none)."""
    import scene_mha_cases as MC
    import test_fusion_table_gpu as FT
    _, O = _mods()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    net = FT._net(config, False)
    rgb, lid, bb, b3, pid = V._fixture_inputs(counts)
    with torch.no_grad(), _Calls() as n:
        res = net(rgb, lid, bb, b3, None, pid)
    assert n.get(ENTRY, 0) == (0 if config == "crossAtt" else 1)
    tag = MC.net_tag(config, counts, "eval")
    for i, r in enumerate(res):
        V.close(r, FT.G["%s_%02d" % (tag, i)], rtol=2e-4)
    for name in ("bn_rgb", "bn_lidar"):
        assert int(getattr(net, name).num_batches_tracked) == 0


def test_graph_capture(monkeypatch):
    """The eval forward of the fusion net captured into a graph and replayed twice equals the eager result bit for bit, group
    ids included (the cached parameter blocks are built by the warm-up call)."""
    _, O = _mods()
    monkeypatch.setattr(O, "SCENE_TAIL_FUSE", True)
    counts = (2, 7, 33, 5, 12)
    batch = V._batch(counts, 21)
    net = V._net("Attention_mat", False)
    net.actor_counts = list(counts)
    with torch.no_grad():
        eager = [o.clone() for o in _forward(net, batch)] + [net._tail_group_id.clone()]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _forward(net, batch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = list(_forward(net, batch)) + [net._tail_group_id]
        for _ in range(2):
            out[0].zero_(); out[-1].zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, eager):
                assert torch.equal(a, b) and torch.equal(a.isnan(), b.isnan())
