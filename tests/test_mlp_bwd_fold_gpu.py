"""Backward of the last two layers of a shared MLP with the max-pool layer's gradient formed inside the conv's dX / dW
kernels (bn_ops._BnActConvBnMaxPool; csrc/pointwise_fwd.hip GRAD mode, csrc/pointwise_dw.hip GRAD instances) instead of
written by bn_max_bwd_apply_kernel and read back twice.

Truth: the same chain -- 1x1 conv -> train-mode BN -> ReLU -> 1x1 conv -> BN -> ReLU -> max over ns -- in float64 torch with
autograd in double.  Compared: the input gradient, both dW, both dgamma and dbeta.  Measure: max |error| against the truth over
the quantity's max |truth|.  Bounds: at most 2x the same measure of the unfolded route (bn_ops.FOLD_MAXPOOL_BWD = False) on the
same inputs -- the same operand values enter the same MFMA chains -- and at most the project's parity bound 1e-4.

How the inputs keep an fp32-against-fp64 comparison meaningful (a ReLU mask or an arg-max that flips between the two precisions
moves a whole gradient entry, in ANY fp32 implementation, folded or not):
  * every group repeats its first column in its last slots, as a padded ball query does: exact ties are the norm, and the
    input gradient is taken at the distinct columns, where the tied slots add up;
  * the input and the first conv's weights are small dyadic numbers, so the first pre-BN tensor is exact in fp32 and the first
    ReLU's mask can only flip if an attainable value lies at the threshold: the test asserts a margin of 1e-4;
  * the upstream gradient is zero in the groups whose float64 arg-max is decided by less than 1e-3 (in units of the
    normalised output) or whose pooled value is that close to the ReLU's zero.
Measured on an MI355X: the folded and the unfolded route are bit-identical in all 7 quantities of all 5 cases (ratio 1.000);
their error over max |truth| lies between 6.4e-8 (dbeta2, ragged) and 1.4e-6 (dbeta1, ragged), the input gradient at 2.1e-7 to
4.2e-7.  The test prints the table."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
C0 = 8            # channels of the grouped input in front of the first conv

# name: B, M, ns, C1 -> C2, distinct columns per group, channel with gamma = 0 and beta < 0, strided dpool + rowmajor grad
CASES = {
    "ob2_p128": dict(B=2, M=1024, ns=32, C1=32, C2=64, K=20, dead=None, stacked=False),     # OB = 2 rows in dW; P % 128 == 0
    "ragged": dict(B=2, M=2050, ns=16, C1=16, C2=32, K=10, dead=5, stacked=False),          # P % 128 = 32
    "ns12": dict(B=3, M=1825, ns=12, C1=20, C2=24, K=7, dead=None, stacked=False),          # ns no power of two; odd channels
    "stacked": dict(B=1, M=4100, ns=16, C1=32, C2=32, K=11, dead=9, stacked=True),          # dpool slice of (M, 96)^T; rowmajor
    "ns6_fallback": dict(B=2, M=5462, ns=6, C1=16, C2=32, K=4, dead=None, stacked=False),   # ns % 4 != 0: the unfolded route
}
NAMES = ["in_grad", "dW1", "dgamma1", "dbeta1", "dW2", "dgamma2", "dbeta2"]
_cache = {}


def _inputs(name):
    c = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    B, M, ns, C1, C2, K = c["B"], c["M"], c["ns"], c["C1"], c["C2"], c["K"]
    base = torch.randint(-3, 4, (B, C0, M, K), generator=gen).float()                     # dyadic: conv 1 is exact in fp32
    idx = torch.cat([torch.arange(K), torch.zeros(ns - K, dtype=torch.long)])             # the padding repeats column 0
    w1 = torch.randint(-8, 9, (C1, C0), generator=gen).float() / 8
    w2 = torch.randn(C2, C1, generator=gen) / C1 ** 0.5
    g1, b1 = torch.rand(C1, generator=gen) + 0.5, torch.randn(C1, generator=gen) * 0.3
    g2, b2 = torch.rand(C2, generator=gen) + 0.5, torch.randn(C2, generator=gen) * 0.3
    if c["dead"] is not None:
        g2[c["dead"]], b2[c["dead"]] = 0.0, -0.5                                          # pooled <= 0 everywhere: ReLU kills it
    gwide = torch.randn(M, 96, generator=gen) if c["stacked"] else None
    g = gwide.t()[None, 32:32 + C2] if c["stacked"] else torch.randn(B, C2, M, generator=gen)
    return dict(base=base, idx=idx, w1=w1, w2=w2, g1=g1, b1=b1, g2=g2, b2=b2, g=g.contiguous(), gwide=gwide)


def _bn64(x, gamma, beta):
    mean = x.mean((0, 2, 3), keepdim=True)
    var = x.var((0, 2, 3), unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def _truth(name, dev="cuda"):
    """-> (inputs with the near-tie groups of g zeroed, float64 output, float64 gradients, margin of the first ReLU)."""
    if name in _cache:
        return _cache[name]
    inp = _inputs(name)
    K = CASES[name]["K"]
    d = {k: (v.to(dev).double() if v is not None and v.is_floating_point() else v) for k, v in inp.items()}
    leaves = [d[k].clone().requires_grad_(True) for k in ("base", "w1", "g1", "b1", "w2", "g2", "b2")]
    base, w1, g1, b1, w2, g2, b2 = leaves
    x = base[..., d["idx"].to(dev)]
    z1 = _bn64(torch.einsum("oi,bims->boms", w1, x), g1, b1)
    z2 = _bn64(torch.einsum("oi,bims->boms", w2, torch.relu(z1)), g2, b2)
    y = torch.relu(z2).max(dim=3).values
    top = z2.detach()[..., :K].topk(2, dim=3).values                                      # the distinct columns
    pooled, gap = top[..., 0], top[..., 0] - top[..., 1]
    unsafe = (pooled.abs() < 1e-3) | ((pooled > 0) & (gap < 1e-3))
    g = d["g"].masked_fill(unsafe, 0.0)
    grads = torch.autograd.grad(y, leaves, g)
    inp["g"] = g.float().cpu()
    if inp["gwide"] is not None:
        inp["gwide"][:, 32:32 + g.shape[1]] = inp["g"][0].t()
    out = (inp, y.detach(), dict(zip(NAMES, [t.detach() for t in grads])), float(z1.detach().abs().min()),
           float(unsafe.double().mean()))
    _cache[name] = out
    return out


def _mlp(inp, C1, C2):
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import shared_mlp_2d
    mlp = shared_mlp_2d([C0, C1, C2]).cuda().train()
    convs = [m for m in mlp if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in mlp if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(convs) == 2 and len(bns) == 2 and all(c.bias is None for c in convs) and all(b.eps == EPS for b in bns)
    with torch.no_grad():
        convs[0].weight.copy_(inp["w1"].view_as(convs[0].weight)); convs[1].weight.copy_(inp["w2"].view_as(convs[1].weight))
        bns[0].weight.copy_(inp["g1"]); bns[0].bias.copy_(inp["b1"])
        bns[1].weight.copy_(inp["g2"]); bns[1].bias.copy_(inp["b2"])
    return mlp, convs, bns


def _forward(mlp, x, stacked):
    from multimodal_gar_amd import nn_utils
    if not stacked:
        return mlp.forward_maxpool(x)
    # the stacked modules run the first conv inside their grouping kernel and enter the MLP at its first BatchNorm, asking for
    # the input gradient as rows
    return mlp.forward_maxpool(nn_utils.conv1x1(mlp[0], x), start=1, rowmajor_input_grad=True)


def _run(name, inp, fold):
    from multimodal_gar_amd import bn_ops
    c = CASES[name]
    mlp, convs, bns = _mlp(inp, c["C1"], c["C2"])
    base = inp["base"].cuda().requires_grad_(True)
    x = base[..., inp["idx"].cuda()]
    g = inp["gwide"].cuda().t()[None, 32:32 + c["C2"]] if c["stacked"] else inp["g"].cuda()
    assert g.is_contiguous() == (not c["stacked"])
    old = bn_ops.FOLD_MAXPOOL_BWD
    bn_ops.FOLD_MAXPOOL_BWD = fold
    try:
        y = _forward(mlp, x, c["stacked"])
        node = y.grad_fn.name()
        y.backward(g)
    finally:
        bn_ops.FOLD_MAXPOOL_BWD = old
    grads = [base.grad, convs[0].weight.grad.view(c["C1"], C0), bns[0].weight.grad, bns[0].bias.grad,
             convs[1].weight.grad.view(c["C2"], c["C1"]), bns[1].weight.grad, bns[1].bias.grad]
    return y.detach(), dict(zip(NAMES, grads)), node


def _measure(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_folded_backward_matches_fp64_no_worse_than_unfolded(name):
    inp, y64, want, margin, zeroed = _truth(name)
    assert margin > 1e-4, "the inputs put a first-layer activation at the ReLU threshold: %g" % margin
    assert zeroed < 0.05
    y_on, on, node_on = _run(name, inp, True)
    y_off, off, node_off = _run(name, inp, False)
    folded = CASES[name]["ns"] % 4 == 0
    assert ("BnActConvBnMaxPool" in node_on) == folded, node_on          # the fold is taken exactly where it applies
    assert "BnActConvBnMaxPool" not in node_off
    assert torch.equal(y_on, y_off), "the forward launches are the same: the outputs must be bit-identical"
    assert _measure(y_on, y64) <= 1e-4
    if CASES[name]["dead"] is not None:
        assert float(y_on[:, CASES[name]["dead"]].max()) == 0.0          # ReLU killed the whole channel
    for q in NAMES:
        e_on, e_off = _measure(on[q], want[q]), _measure(off[q], want[q])
        print("%-13s %-8s folded %.3e  unfolded %.3e  ratio %s  bit-identical %s" % (
            name, q, e_on, e_off, "%.3f" % (e_on / e_off) if e_off > 0 else "-", torch.equal(on[q], off[q])))
    for q in NAMES:
        e_on, e_off = _measure(on[q], want[q]), _measure(off[q], want[q])
        assert e_on <= 2 * e_off, (q, e_on, e_off)
        assert e_on <= 1e-4, (q, e_on)


def test_folded_backward_replays_from_a_captured_graph_bit_for_bit():
    name = "ragged"
    inp = _truth(name)[0]
    c = CASES[name]
    y_eager, eager, node = _run(name, inp, True)
    assert "BnActConvBnMaxPool" in node
    mlp, convs, bns = _mlp(inp, c["C1"], c["C2"])
    params = [convs[0].weight, bns[0].weight, bns[0].bias, convs[1].weight, bns[1].weight, bns[1].bias]
    base = inp["base"].cuda().requires_grad_(True)
    idx, g = inp["idx"].cuda(), inp["g"].cuda()

    def step():
        for t in [base] + params:
            t.grad = None
        y = mlp.forward_maxpool(base[..., idx])
        y.backward(g)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for t in [base] + params:
        t.grad = None
    with torch.cuda.graph(graph):
        y = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y_eager)
    got = [base.grad, convs[0].weight.grad.view(c["C1"], C0), bns[0].weight.grad, bns[0].bias.grad,
           convs[1].weight.grad.view(c["C2"], c["C1"]), bns[1].weight.grad, bns[1].bias.grad]
    for q, t in zip(NAMES, got):
        assert torch.equal(t, eager[q]), q
