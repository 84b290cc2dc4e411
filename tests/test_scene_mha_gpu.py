"""Per-scene multi-head attention core (csrc/scene_mha.hip) against the float64 reference of tests/scene_mha_cases.py:
forward and both backward passes at the cases of its table (out, att, dq, dk, dv within RTOL of the comparator's largest
entry + ATOL), Att rows summing to 1, identical bits on two runs, refusals that write nothing, and
scene_multihead_attention against nn.MultiheadAttention's own unbatched call, scene by scene, on the device."""
import functools

import pytest
import torch

import scene_mha_cases as MC

pytestmark = pytest.mark.gpu
SCALE = 1.0 / MC.HEAD_DIM ** 0.5


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = MC.CASES[name]
    q, k, v, grad = MC.inputs(case["counts"], case["H"], case.get("qk_scale", 1.0))
    return (q, k, v, grad), MC.mha_reference(q, k, v, case["counts"], case["H"], SCALE, grad)


def _device_inputs(name):
    """q, k, v on the device at the case's leading dimension (column slices of wider buffers), requiring gradients."""
    case = MC.CASES[name]
    (q, k, v, grad), _ = _reference(name)
    rows, D, ld = q.shape[0], q.shape[1], case["ld"]
    if case.get("fused"):
        buf = torch.cat((q, k, v), dim=1).cuda().requires_grad_(True)
        assert buf.shape[1] == ld
        return buf, tuple(buf[:, i * D:(i + 1) * D] for i in range(3)), grad.cuda()
    bufs = [torch.full((rows, ld), 7.0).cuda() for _ in range(3)]       # what lies beside the heads must not be read
    for b, t in zip(bufs, (q, k, v)):
        b[:, :D] = t.cuda()
        b.requires_grad_(True)
    return bufs, tuple(b[:, :D] for b in bufs), grad.cuda()


def _run(name):
    from multimodal_gar_amd.dafm_ops import scene_offsets
    from multimodal_gar_amd.scene_mha_ops import scene_mha
    case = MC.CASES[name]
    counts = case["counts"]
    leaves, (q, k, v), grad = _device_inputs(name)
    so, do = scene_offsets(counts, q.device)
    out, att = scene_mha(q, k, v, so, do, sum(n * n for n in counts), case["H"], SCALE)
    out.backward(grad)
    D = q.shape[1]
    if case.get("fused"):
        g = leaves.grad
        grads = tuple(g[:, i * D:(i + 1) * D] for i in range(3))
    else:
        grads = tuple(b.grad[:, :D] for b in leaves)
        for b in leaves:
            assert not b.grad[:, D:].any()
    return (out.detach(), att) + grads


def _close(got, want, what):
    want = want.to(torch.float64)
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.numel() == 0:
        return
    err, bound = float((got - want).abs().max()), MC.RTOL * float(want.abs().max()) + MC.ATOL
    print("%s: max err %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_forward_and_backward_match_float64(name):
    case = MC.CASES[name]
    got = _run(name)
    _, want = _reference(name)
    for g, w, what in zip(got, want, ("out", "att", "dq", "dk", "dv")):
        _close(g, w, "%s %s" % (name, what))
    att, m0 = got[1], 0
    assert att.shape == (case["H"], sum(n * n for n in case["counts"]))
    for n in case["counts"]:                                 # every row of every scene and head sums to 1
        if n:
            sums = att[:, m0:m0 + n * n].reshape(case["H"], n, n).sum(dim=2)
            assert float((sums - 1).abs().max()) <= 1e-5
        m0 += n * n


@pytest.mark.parametrize("name", ["n128_n127_H8_fused", "empty_scenes_H1"])
def test_two_runs_give_identical_bits(name):
    a, b = _run(name), _run(name)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_write_nothing_and_empty_is_ok():
    from multimodal_gar_amd import _lib as L
    from multimodal_gar_amd.dafm_ops import scene_offsets
    counts, H = [3, 2], 2
    rows, pairs = sum(counts), sum(n * n for n in counts)
    so, do = scene_offsets(counts, "cuda")
    x = torch.randn(rows, 136, device="cuda")
    att, gmat = torch.full((H, pairs), 5.0, device="cuda"), torch.full((H, pairs), 5.0, device="cuda")
    outs = [torch.full((rows, 128), 5.0, device="cuda") for _ in range(4)]
    st = L.stream_of(x)
    for hd, ld in ((32, 128), (64, 130)):
        rc = L._fns["mgar_scene_mha_fwd"](len(counts), rows, H, hd, L.iptr(so), L.iptr(do), pairs, L.fptr(x), L.fptr(x), L.fptr(x),
                                          ld, SCALE, L.fptr(att), L.fptr(outs[0]), st)
        assert rc == -3
        rc = L._fns["mgar_scene_mha_bwd"](len(counts), rows, H, hd, L.iptr(so), L.iptr(do), pairs, L.fptr(x), L.fptr(x), L.fptr(x),
                                          ld, SCALE, L.fptr(att), L.fptr(outs[0]), L.fptr(gmat), L.fptr(outs[1]),
                                          L.fptr(outs[2]), L.fptr(outs[3]), st)
        assert rc == -3
        with pytest.raises(L.MgarError):
            L.call("mgar_scene_mha_fwd", len(counts), rows, H, hd, L.iptr(so), L.iptr(do), pairs, L.fptr(x), L.fptr(x),
                   L.fptr(x), ld, SCALE, L.fptr(att), L.fptr(outs[0]), st)
    torch.cuda.synchronize()
    for t in [att, gmat] + outs:
        assert bool((t == 5.0).all())
    so0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L._fns["mgar_scene_mha_fwd"](0, 0, H, 64, L.iptr(so0), None, 0, None, None, None, 128, SCALE, None, None, st) == 0
    # the op layer on an empty batch of scenes
    from multimodal_gar_amd.scene_mha_ops import scene_mha
    e = torch.zeros(0, 128, device="cuda")
    out, a = scene_mha(e, e, e, so0, torch.zeros(0, dtype=torch.int32, device="cuda"), 0, H, SCALE)
    assert out.shape == (0, 128) and a.shape == (H, 0)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_scene_multihead_attention_matches_the_module_per_scene(kind):
    """Outputs and parameter gradients against mha(query, key, value)[0] called unbatched on every scene.
    The bound is the DAFM op tolerance once for each fp32 side, 2 * (RTOL * max + ATOL).  Observed on an MI355X, largest
    error / bound: outputs 8.3e-7 / 2.1e-4, input gradients 8.3e-7 / 2.5e-4, in_proj_weight 7.2e-6 / 1.7e-3, in_proj_bias
    3.3e-6 / 2.5e-3, out_proj.weight 6.2e-6 / 2.1e-3, out_proj.bias 2.4e-6 / 4.2e-3 -- a few ulp of each tensor's largest
    entry, two orders of magnitude inside the bound."""
    from multimodal_gar_amd.dafm_ops import scene_offsets
    from multimodal_gar_amd.scene_mha_ops import scene_multihead_attention
    counts = [2, 7, 33]
    g = torch.Generator().manual_seed(5)
    x, y, grad = (torch.randn(sum(counts), 512, generator=g).cuda() for _ in range(3))
    torch.manual_seed(7)
    mha = torch.nn.MultiheadAttention(512, 8).cuda()
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.1)
        mha.out_proj.bias.normal_(0, 0.1)
    so, do = scene_offsets(counts, x.device)

    def run(packed):
        mha.zero_grad(set_to_none=True)
        xq, ym = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        mem = xq if kind == "self" else ym
        if packed:
            out = scene_multihead_attention(mha, xq, mem, mem, so, do, sum(n * n for n in counts))
        else:
            outs, r0 = [], 0
            for n in counts:
                outs.append(mha(xq[r0:r0 + n], mem[r0:r0 + n], mem[r0:r0 + n])[0])
                r0 += n
            out = torch.cat(outs)
        out.backward(grad)
        res = {"out": out.detach(), "query": xq.grad}
        if kind == "cross":
            res["memory"] = ym.grad
        res.update({n: p.grad.clone() for n, p in mha.named_parameters()})
        return res
    got, want = run(True), run(False)
    assert set(got) == set(want) and len(got) >= 6
    for key in want:
        # fp32 against fp32: the DAFM op tests' tolerance on each side of the comparison
        err = float((got[key].double() - want[key].double()).abs().max())
        bound = 2 * (MC.RTOL * float(want[key].abs().max()) + MC.ATOL)
        print("%s %s: max err %.3e, bound %.3e" % (kind, key, err, bound))
        assert err <= bound, (key, err, bound)
