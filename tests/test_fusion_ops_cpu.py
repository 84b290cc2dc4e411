"""Fusion-head ops (csrc/gatv2.hip, csrc/dafm.hip, csrc/roi_align.hip) -- what can be pinned without a GPU.

The device test (tests/test_fusion_edges_gpu.py) judges the kernels by the float64 references in torch_refs.py at the
inputs of fusion_cases.py.  Here, with no kernel involved:

* `edges_to_csr` / `csr_by_source` (pure torch, they feed the kernels their index arrays) against a brute-force Python
  construction, with the properties the atomics-free backward's bit-reproducibility rests on;
* the float64 references agree with the oracle (an independent restatement) on the new sparse, non-square and boundary
  cases, so a kernel is never judged by a reference that was not itself checked;
* the rebuilt `roi_align_ref` (bins summed one by one) equals the former one (a running (C, ph, pw) accumulator), values
  and input gradient, to 1e-12;
* every RoI of every case keeps a distance >= 1e-3 from every discontinuity of RoIAlign (fp32 coordinate error at
  |coordinate| <= 64 is below 1e-5), so fp32 and float64 take the same samples;
* a scene above the DAFM kernels' capacity is rejected on the host."""
import math

import numpy as np
import pytest
import torch

import fusion_cases as FC
import torch_refs as R


# ------------------------------------------------------------------------------------------------ CSR
def _brute_csr(edge_index, n, add_self_loops):
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    pairs = list(zip(src, dst))
    if add_self_loops:
        pairs = [(j, i) for j, i in pairs if j != i] + [(i, i) for i in range(n)]
    rowptr, col = [0], []
    for i in range(n):
        col += [j for j, t in pairs if t == i]          # list order within a target
        rowptr.append(len(col))
    return rowptr, col


GRAPHS = [("complete5", lambda: FC.complete_graph(5), 5), ("sparse_dups", lambda: FC.sparse_graph(40, duplicates=True), 40),
          ("sparse", lambda: FC.sparse_graph(40, duplicates=False), 40), ("holes", lambda: FC.holes_graph(12), 12),
          ("random_n17_e90", lambda: FC.random_graph(17, 90, 1), 17), ("random_n64_e300", lambda: FC.random_graph(64, 300, 2), 64),
          ("random_noloops", lambda: FC.random_graph(9, 40, 3, loops=False), 9), ("n1_loop", lambda: torch.zeros((2, 3), dtype=torch.int64), 1),
          ("n1_E0", lambda: FC.random_graph(1, 0, 0), 1), ("n6_E0", lambda: FC.random_graph(6, 0, 0), 6)]


@pytest.mark.parametrize("add_self_loops", [True, False])
@pytest.mark.parametrize("name,make,n", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_csr_matches_brute_force_and_by_source_properties(name, make, n, add_self_loops):
    from multimodal_gar_amd.graph_ops import csr_by_source, edges_to_csr
    ei = make()
    rowptr, col = edges_to_csr(ei, n, add_self_loops)
    want_rowptr, want_col = _brute_csr(ei, n, add_self_loops)
    assert rowptr.dtype == col.dtype == torch.int32
    assert rowptr.tolist() == want_rowptr and col.tolist() == want_col
    E = len(want_col)
    if add_self_loops:                                   # exactly one loop per node, the last edge of its target
        for i in range(n):
            assert col[rowptr[i + 1] - 1].item() == i and want_col[want_rowptr[i]:want_rowptr[i + 1]].count(i) == 1
    src_rowptr, src_edge, src_dst = csr_by_source(rowptr, col)
    assert src_rowptr.dtype == src_edge.dtype == src_dst.dtype == torch.int32
    assert src_rowptr.numel() == n + 1 and src_rowptr[0].item() == 0 and src_rowptr[-1].item() == E
    assert sorted(src_edge.tolist()) == list(range(E))                       # a permutation of 0 .. E-1
    target_of = [i for i in range(n) for _ in range(want_rowptr[i], want_rowptr[i + 1])]
    sr, se, sd = src_rowptr.tolist(), src_edge.tolist(), src_dst.tolist()
    for j in range(n):
        ids = se[sr[j]:sr[j + 1]]
        assert ids == sorted(ids)                                           # ascending edge ids within a source
        assert ids == [e for e in range(E) if want_col[e] == j]             # exactly j's outgoing edges
        assert sd[sr[j]:sr[j + 1]] == [target_of[e] for e in ids]           # and their targets


def test_case_graphs_have_the_structure_their_cases_are_there_for():
    from multimodal_gar_amd.graph_ops import csr_by_source, edges_to_csr
    dups, plain = FC.sparse_graph(40, duplicates=True), FC.sparse_graph(40, duplicates=False)
    as_pairs = lambda g: list(zip(g[0].tolist(), g[1].tolist()))            # noqa: E731
    assert len(set(as_pairs(plain))) == plain.shape[1] and set(as_pairs(plain)) == set(as_pairs(dups))
    assert dups.shape[1] == plain.shape[1] + 30
    assert as_pairs(plain) != sorted(as_pairs(plain))                       # unsorted
    assert any(j > i for j, i in as_pairs(plain)) and set(as_pairs(plain)) != {(i, j) for j, i in as_pairs(plain)}   # asymmetric
    for j in FC.SPARSE_INPUT_LOOPS:
        assert (j, j) in as_pairs(plain)
    rowptr, col = edges_to_csr(dups, 40, True)
    sr = csr_by_source(rowptr, col)[0].tolist()
    for j in FC.SPARSE_SILENT_SOURCES:
        assert sr[j + 1] - sr[j] == 1                                       # the re-added self loop only
    holes = FC.holes_graph(12)
    rowptr, col = edges_to_csr(holes, 12, False)
    rp, sr = rowptr.tolist(), csr_by_source(rowptr, col)[0].tolist()
    for i in range(12):
        assert (rp[i + 1] == rp[i]) == (i in FC.HOLES_NO_INCOMING)
    for j in FC.HOLES_NO_OUTGOING:
        assert sr[j + 1] == sr[j]
    assert 7 in col[rp[7]:rp[8]].tolist()                                    # the input self loop stays an edge


# ------------------------------------------------------------------------------------------------ references vs oracle
def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)


@pytest.mark.parametrize("name", [k for k, c in FC.GAT_CASES.items() if not c.get("train")])
def test_gatv2_ref_matches_oracle(oracle, name):
    from multimodal_gar_amd.graph_ops import GATv2Conv, edges_to_csr
    case = FC.GAT_CASES[name]
    n, H, C = case["n"], case["H"], case["C"]
    opts = dict(concat=case.get("concat", False), add_self_loops=case.get("add_self_loops", True), bias=case.get("bias", True),
                share_weights=case.get("share_weights", False))
    torch.manual_seed(2)
    conv = GATv2Conv(C, C, H, dropout=0.5, **opts).double().eval()
    with torch.no_grad():                               # non-zero biases, so that a dropped bias shows
        for p in (conv.lin_l.bias, conv.lin_r.bias, conv.bias):
            if p is not None:
                p.uniform_(-0.5, 0.5)
    x = torch.randn(n, C, dtype=torch.float64)
    ei = FC.gat_graph(case["graph"], n)
    out, alpha = R.gatv2_ref(x, ei, conv.lin_l, conv.lin_r, conv.att, conv.bias, H, C, concat=opts["concat"],
                             add_self_loops=opts["add_self_loops"], share_weights=opts["share_weights"], return_alpha=True)
    zeros = np.zeros(H * C)
    npy = lambda t: zeros if t is None else t.detach().numpy()             # noqa: E731
    want = oracle.gatv2(x.numpy(), ei.numpy(), npy(conv.lin_l.weight), npy(conv.lin_l.bias), npy(conv.lin_r.weight),
                        npy(conv.lin_r.bias), npy(conv.att), 0.0 if conv.bias is None else npy(conv.bias), H, C,
                        concat=opts["concat"], add_self_loops=opts["add_self_loops"])
    assert out.shape == want.shape and _rel(out, want) <= 1e-12
    # alpha: CSR edge order, one softmax per (target, head)
    rowptr, col = edges_to_csr(ei, n, opts["add_self_loops"])
    assert alpha.shape == (col.numel(), H)
    rp = rowptr.tolist()
    for i in range(n):
        if rp[i + 1] > rp[i]:
            assert (alpha[rp[i]:rp[i + 1]].sum(0) - 1).abs().max().item() <= 1e-12
    if not opts["add_self_loops"]:
        for i in FC.HOLES_NO_INCOMING:                  # nothing aggregated: the row is the bias
            assert torch.equal(out[i], conv.bias.detach())


def test_gatv2_ref_keeps_duplicate_edges_as_duplicates():
    """Two copies of j -> i weigh twice in i's softmax (PyG does not coalesce)."""
    torch.manual_seed(0)
    lin_l, lin_r = torch.nn.Linear(64, 64).double(), torch.nn.Linear(64, 64).double()
    att = torch.randn(1, 1, 64, dtype=torch.float64)
    x = torch.randn(3, 64, dtype=torch.float64)
    _, a1 = R.gatv2_ref(x, torch.tensor([[0, 1], [2, 2]]), lin_l, lin_r, att, None, 1, 64, return_alpha=True)
    _, a2 = R.gatv2_ref(x, torch.tensor([[0, 1, 0], [2, 2, 2]]), lin_l, lin_r, att, None, 1, 64, return_alpha=True)
    t1, t2 = a1[2:], a2[2:]                              # target 2: [0, 1, loop] and [0, 1, 0, loop]
    assert t2.shape[0] == 4 and torch.allclose(t2[0], t2[2], rtol=0, atol=1e-15)
    assert torch.allclose(t2[0] / t2[1], t1[0] / t1[1], rtol=1e-12) and (t2[0] + t2[2] > t1[0]).all()


@pytest.mark.parametrize("name", list(FC.DAFM_CASES))
def test_dafm_ref_matches_oracle(oracle, name):
    case = FC.DAFM_CASES[name]
    counts, D = case["counts"], case["D"]
    q, k, v, des, _ = FC.dafm_inputs(counts, D, case.get("de_max", 20.0), case.get("qk_scale", 1.0))
    scale, r0 = 1.0 / D ** 0.5, 0
    for n, de in zip(counts, des):
        if n:
            sl = slice(r0, r0 + n)
            out, att = R.dafm_ref(q[sl].double(), k[sl].double(), v[sl].double(), de.double(), FC.DAFM_SIGMA, scale)
            o_np, a_np = oracle.dafm_attention(q[sl].numpy(), k[sl].numpy(), v[sl].numpy(), de.numpy(), FC.DAFM_SIGMA, scale)
            assert _rel(out, o_np) <= 1e-12 and _rel(att, a_np) <= 1e-12
            assert (att.sum(1) - 1).abs().max().item() <= 1e-12
        r0 += n
    if name == "e_underflow":                           # what the case is there for: fp32 E has exact zeros off the diagonal
        e32 = torch.softmax(-(des[0] / FC.DAFM_SIGMA), dim=1)
        assert (e32 == 0).float().mean().item() > 0.3 and (e32.diagonal() > 0).all()


@pytest.fixture(scope="module")
def roi_cases():
    return {name: make() for name, make in FC.ROI_CASES.items()}


@pytest.mark.parametrize("name", list(FC.ROI_CASES))
def test_roi_align_ref_matches_oracle(oracle, roi_cases, name):
    c = roi_cases[name]
    ref = R.roi_align_ref(torch.from_numpy(c["feat"]), torch.from_numpy(c["rois"]), c["out_size"], c["scale"],
                          c["sampling_ratio"], c["aligned"])
    want = torch.from_numpy(oracle.roi_align(c["feat"], c["rois"], c["out_size"], c["scale"], c["sampling_ratio"], c["aligned"]))
    assert ref.shape == want.shape
    err, top = (ref - want.double()).abs().max().item(), ref.abs().max().item()
    assert err <= 1e-5 + 1e-4 * top, (err, top)         # the oracle is fp32 C: the device test's tolerance
    if name == "degenerate_aligned":
        assert (ref[list(FC.ROI_DEGENERATE_ZERO_OUTPUT)] == 0).all() and ref[5].abs().max().item() > 0.1


def test_roi_cases_sizes():
    c = FC.roi_grid_stride()
    K, C = c["rois"].shape[0], c["feat"].shape[1]
    assert K == 202 and K * C * 25 == 4201600 == 16384 * 256 + 7296
    pad = (c["rois"][:, 1:] == 0).all(1)
    assert pad.sum() == 52 and set(c["rois"][pad, 0]) == {0.0, 1.0}
    x1, y1, x2, y2 = c["rois"][~pad, 1:].T
    assert ((x1 < 0) | (y1 < 0) | (x2 > 160) | (y2 > 96)).sum() >= 50       # reach outside the 160 x 96 px image
    c = FC.roi_contended()
    assert (c["rois"][:64] == c["rois"][0]).all() and len(np.unique(c["rois"], axis=0)) == 65
    for size in ((3, 7), (7, 3)):
        assert (FC.roi_non_square(size)["rois"][:, 0] == 2).sum() >= 3


@pytest.mark.parametrize("name", list(FC.ROI_CASES))
def test_roi_inputs_stay_clear_of_the_discontinuities(roi_cases, name):
    """RoIAlign jumps where a sample coordinate crosses -1, H or W (the sample is dropped) and where rh / ph or rw / pw
    crosses an integer (ceil changes the sample count).  Every RoI of every case -- the padded all-zero boxes too: rw = rh =
    1, one sample at 0.1 -- stays >= 1e-3 away in float64.  One extent is exempt from the integer condition by
    construction, not by margin: the zero-area box of the aligned case has x2 == x1 and y2 == y1 as numbers, so its extent
    is 0 and its sample count 0 in every precision; that is asserted below instead."""
    c = roi_cases[name]
    _, _, H, W = c["feat"].shape
    d = FC.roi_clearance(c["rois"], H, W, c["out_size"], c["scale"], c["sampling_ratio"], c["aligned"])
    assert d.shape == (len(c["rois"]),)
    print("%s: smallest clearance %.3e over %d RoIs" % (name, d.min(), len(d)))
    assert d.min() >= FC.CLEARANCE, (int(d.argmin()), d.min())
    assert math.frexp(c["scale"])[0] == 0.5              # a power of two: box * scale is exact in fp32
    if c["aligned"]:
        r = c["rois"]
        same = (r[:, 1] == r[:, 3]) | (r[:, 2] == r[:, 4])
        for row in r[same]:                              # fp32 arithmetic of the kernel: exactly 0
            off = np.float32(0.5)
            s = np.float32(c["scale"])
            assert (row[3] * s - off) - (row[1] * s - off) == 0 and (row[4] * s - off) - (row[2] * s - off) == 0


# ------------------------------------------------------------------------------------------------ roi_align_ref, rebuilt
def _roi_align_ref_running_accumulator(inp, rois, out_size, scale, sampling_ratio=-1, aligned=False):
    """torch_refs.roi_align_ref as it was before it summed bin by bin (kept here as the yardstick of the rebuild)."""
    inp = inp.double()
    K = rois.shape[0]
    _, C, H, W = inp.shape
    ph = pw = out_size
    out = []
    off = 0.5 if aligned else 0.0
    for k in range(K):
        b = int(rois[k, 0].item())
        x1, y1, x2, y2 = [float(v) * scale - off for v in rois[k, 1:]]
        rw, rh = x2 - x1, y2 - y1
        if not aligned:
            rw, rh = max(rw, 1.0), max(rh, 1.0)
        bw, bh = rw / pw, rh / ph
        gh = sampling_ratio if sampling_ratio > 0 else math.ceil(rh / ph)
        gw = sampling_ratio if sampling_ratio > 0 else math.ceil(rw / pw)
        acc = torch.zeros((C, ph, pw), dtype=torch.float64, device=inp.device)
        for p_h in range(ph):
            for p_w in range(pw):
                for iy in range(gh):
                    y = y1 + p_h * bh + (iy + 0.5) * bh / gh
                    for ix in range(gw):
                        x = x1 + p_w * bw + (ix + 0.5) * bw / gw
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yy, xx = max(y, 0.0), max(x, 0.0)
                        yl, xl = int(yy), int(xx)
                        if yl >= H - 1:
                            yh = yl = H - 1; yy = float(yl)
                        else:
                            yh = yl + 1
                        if xl >= W - 1:
                            xh = xl = W - 1; xx = float(xl)
                        else:
                            xh = xl + 1
                        ly, lx = yy - yl, xx - xl
                        hy, hx = 1 - ly, 1 - lx
                        acc[:, p_h, p_w] = acc[:, p_h, p_w] + hy * hx * inp[b, :, yl, xl] + hy * lx * inp[b, :, yl, xh] \
                            + ly * hx * inp[b, :, yh, xl] + ly * lx * inp[b, :, yh, xh]
        out.append(acc / max(gh * gw, 1))
    return torch.stack(out)


def _existing_roi_inputs():
    """The inputs of test_fusion_ops_gpu.py's two RoIAlign tests."""
    rng = np.random.default_rng(0)
    feat = torch.from_numpy(rng.standard_normal((2, 7, 12, 20)).astype(np.float32))
    rois = torch.tensor([[0, 3.0, 5.0, 150.0, 100.0], [1, 0.0, 0.0, 319.0, 191.0], [0, 200.0, 40.0, 210.0, 44.0],
                         [1, 0.0, 0.0, 0.0, 0.0], [0, 300.0, 180.0, 330.0, 200.0], [1, -20.0, -10.0, 50.0, 60.0]])
    yield feat, rois, 5, 1 / 16.0, -1, False
    yield feat, rois, 3, 0.0625, 2, True
    torch.manual_seed(0)
    feat = torch.randn(2, 5, 9, 14, dtype=torch.float32)
    rois = torch.tensor([[0, 4.0, 4.0, 100.0, 90.0], [0, 0.0, 0.0, 0.0, 0.0], [1, 30.0, 10.0, 200.0, 120.0]])
    yield feat, rois, 5, 14 / 224.0, -1, False


def test_roi_align_ref_rebuilt_equals_running_accumulator():
    for feat, rois, size, scale, sr, aligned in _existing_roi_inputs():
        grads, outs = [], []
        for fn in (R.roi_align_ref, _roi_align_ref_running_accumulator):
            f = feat.double().requires_grad_(True)
            out = fn(f, rois, size, scale, sr, aligned)
            g = torch.linspace(-1, 1, out.numel(), dtype=torch.float64).view(out.shape)
            out.backward(g)
            outs.append(out.detach()); grads.append(f.grad)
        assert outs[0].shape == outs[1].shape
        assert (outs[0] - outs[1]).abs().max().item() <= 1e-12 and (grads[0] - grads[1]).abs().max().item() <= 1e-12
        assert torch.equal(R.roi_align_ref(feat, rois, (size, size), scale, sr, aligned), outs[0])     # the pair form


# ------------------------------------------------------------------------------------------------ DAFM capacity
def test_dafm_capacity_is_read_from_the_header_and_enforced_on_the_host():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import scene_offsets
    with open(L.HEADER_PATH) as f:
        assert "#define MGAR_DAFM_MAX_N %d\n" % L.DAFM_MAX_N in f.read()
    so, do = scene_offsets([L.DAFM_MAX_N, 0, 1], "cpu")                      # the limit itself and an empty scene pass
    assert so.tolist() == [0, L.DAFM_MAX_N, L.DAFM_MAX_N, L.DAFM_MAX_N + 1]
    assert do.tolist() == [0, L.DAFM_MAX_N ** 2, L.DAFM_MAX_N ** 2]
    for counts in ([L.DAFM_MAX_N + 1], [3, L.DAFM_MAX_N + 1, 5], [129]):
        with pytest.raises(ValueError, match=r"\b%d\b.*MGAR_DAFM_MAX_N" % L.DAFM_MAX_N):
            scene_offsets(counts, "cpu")
    with pytest.raises(ValueError):
        scene_offsets([4, -1], "cpu")
