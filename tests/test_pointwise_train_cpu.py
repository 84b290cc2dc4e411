"""What tests/test_pointwise_train_gpu.py rests on, checked with no kernel: the float64 references of
tests/pointwise_train_cases.py are torch's float64 autograd of the same expressions; the restated launch geometry gives the
library's own workspace sizes; every instance and path of the three files is reached by a case; the exact cases are exact; an
fp32 evaluation of each bounded case lies inside its bound; and a plausible kernel bug -- a dropped column, a dropped tail
tile, an arg one slot off, m0 and m1 swapped, a ReLU left out, W read untransposed, a reduce slice lost -- leaves it."""
import numpy as np
import pytest
import torch

import pointwise_train_cases as PC

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.asarray(a, F64))   # noqa: E731


def _fn(name):
    from multimodal_gar_amd import _lib
    return _lib._fns[name]


def _bn_t(x, k, relu, prefix=""):
    """The prologue in torch float64 (leaves gamma, beta where given)."""
    if k[prefix + "mean"] is None:
        return x, None, None
    C = x.shape[1]
    g = (T(np.ones(C)) if k[prefix + "gamma"] is None else T(k[prefix + "gamma"])).requires_grad_()
    b = (T(np.zeros(C)) if k[prefix + "beta"] is None else T(k[prefix + "beta"])).requires_grad_()
    a = (x - T(k[prefix + "mean"]).view(1, C, 1)) * T(k[prefix + "invstd"]).view(1, C, 1) * g.view(1, C, 1) + b.view(1, C, 1)
    return (torch.relu(a) if relu else a), g, b


def _close(got, want, what):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert np.abs(got - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0), what


# ------------------------------------------------------------------------------------------------ references = autograd
@pytest.mark.parametrize("name", ["b_ci17_co33_b3_p260", "b_ci16_co32_b3_p132", "b_ci15_co33_b3_p132_wt"])
def test_forward_reference_is_the_conv_of_the_activated_input_and_its_data_gradient(name):
    k = PC.fwd_case(name)
    ref = PC.fwd_ref(k)
    if k["wt"]:      # the buffer is the weight V (Cin, Cout) of a conv from Cout to Cin channels; x is the gradient of its output
        buf, rs, cs = PC.w_buffer(k)
        assert (rs, cs) == (1, k["Cout"])
        u = torch.zeros((k["B"], k["Cout"], k["P"]), dtype=torch.float64, requires_grad=True)
        torch.einsum("io,bop->bip", T(buf), u).backward(T(k["x"]))
        _close(ref["y"], u.grad.numpy(), name)
    else:
        a, _, _ = _bn_t(T(k["x"]), k, k["relu"])
        _close(ref["y"], torch.nn.functional.conv1d(a, T(k["w"])[:, :, None]).detach().numpy(), name)


@pytest.mark.parametrize("name", ["b_ci33_co33_b3_p260", "b_ci64_co32_b1_p131", "b_ci16_co130_b1_p516"])
def test_dw_reference_is_autograd_of_the_weight(name):
    k = PC.dw_case(name)
    a, _, _ = _bn_t(T(k["x"]), k, k["relu"])
    w = torch.zeros((k["Cout"], k["Cin"]), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv1d(a, w[:, :, None]).backward(T(k["dy"]))
    _close(PC.dw_ref(k)["dw"], w.grad.numpy(), name)


@pytest.mark.parametrize("name", sorted(n for n in PC.PAIR_CASES if n.startswith("b_")))
def test_pair_reference_is_autograd_through_bn_relu_conv(name):
    k = PC.pair_case(name)
    a, g, b = _bn_t(T(k["x"]), k, k["relu"])
    w = T(k["w"]).requires_grad_()
    torch.nn.functional.conv1d(a, w[:, :, None]).backward(T(k["dy"]))
    ref = PC.pair_ref(k)
    _close(ref["dw"], w.grad.numpy(), name + " dw")
    _close(ref["dgamma"], g.grad.numpy(), name + " dgamma")
    _close(ref["dbeta"], b.grad.numpy(), name + " dbeta")
    _close(ref["coef"] * k["B"] * k["P"], np.stack([b.grad.numpy(), g.grad.numpy()], 1), name + " coef")


@pytest.mark.parametrize("name", ["b_ns12_m11", "b_ns252_m1", "b_ns128_m11"])
def test_dx4_reference_is_autograd_through_training_batchnorm_relu_max(name):
    """With coef = the means of dz and dz xhat and float64 batch statistics, dx4_ref is the gradient of
    max over ns of relu(batch_norm(x4, training)) -- and the two consumers are the conv's data and weight gradients of it."""
    k = dict(PC.grad_case(name))
    B, C, M, ns, P = k["B"], k["C"], k["M"], k["ns"], k["P"]
    x4 = T(k["x4"]).requires_grad_()
    m, v = PC.BC.stats_of(k["x4"].reshape(B, C, P))
    k.update(mean=m, invstd=(v + PC.BC.EPS) ** -0.5)
    g = None if k["gamma"] is None else T(k["gamma"])
    bn = torch.nn.functional.batch_norm(x4.reshape(B, C, P), None, None, g, T(k["beta"]), True, 0.1, PC.BC.EPS).reshape(B, C, M, ns)
    pre = bn.detach().numpy()
    pooled, arg = PC.R.bn_max_ref(pre, 1)
    out = torch.relu(bn.gather(3, torch.from_numpy(arg)[..., None]).squeeze(3))
    out.backward(T(k["dpool"]))
    dmask = np.where(pooled > 0, k["dpool"].astype(F64), 0.0)
    dz = np.zeros((B, C, M, ns))
    np.put_along_axis(dz, arg[..., None], dmask[..., None], -1)
    r = PC.R.bn_bwd_ref(dz.reshape(B, C, P), k["x4"].reshape(B, C, P), k["mean"], k["invstd"], k["gamma"])
    k.update(mean=np.asarray(k["mean"]), invstd=np.asarray(k["invstd"]), arg=arg)
    dx, _ = PC.dx4_ref(k, r["coef"], dmask)
    _close(dx, x4.grad.numpy().reshape(B, C, P), name)
    _close(dx, r["dx"], name + " torch_refs")
    # consumers: x -> act -> conv W (C, Cp) gives x4; dX of the activated input = W^T dx4, dW = sum dx4 act(x)
    a, _, _ = _bn_t(T(k["x"]), k, k["relu"], "in_")
    a = a.detach().requires_grad_()
    w = T(k["w"]).requires_grad_()
    torch.nn.functional.conv1d(a, w[:, :, None]).backward(T(dx))
    _close(PC.fwd_maxgrad_ref(k, r["coef"], dmask)["y"], a.grad.numpy(), name + " dX")
    _close(PC.dw_maxgrad_ref(k, r["coef"], dmask)["dw"], w.grad.numpy(), name + " dW")


def test_rowmajor_reference():
    k = PC.rd_case("b_co33_ci65_n300")
    a = T(k["a"][:, :33])
    w = torch.zeros((33, 65), dtype=torch.float64, requires_grad=True)
    (T(k["f"][:, :65]) @ w.t()).backward(a)
    _close(PC.rd_ref(k)["dw"], w.grad.numpy(), "rowmajor")


def test_autograd_nan_sets_of_bn_relu_conv():
    """One NaN in x[b, i, p] under in_relu = 1: dW[:, i] and dgamma[i] NaN, dbeta finite, everything else finite -- what
    mgar_pointwise_conv_dw_bnbwd has to return (torch's ReLU backward lets the gradient of a NaN input through)."""
    k = dict(PC.pair_case("b_ci17_co33_b3_p131"))
    x = k["x"].copy()
    b, i, p = k["B"] - 1, 5, k["P"] - 3
    x[b, i, p] = np.nan
    a, g, bt = _bn_t(T(x), k, 1)
    w = T(k["w"]).requires_grad_()
    torch.nn.functional.conv1d(a, w[:, :, None]).backward(T(k["dy"]))
    dw, dg, db = (np.isnan(t.grad.numpy()) for t in (w, g, bt))
    want = np.zeros_like(dw)
    want[:, i] = True
    assert np.array_equal(dw, want) and np.array_equal(dg, want[0]) and not db.any()
    ref = PC.pair_ref(k, force_on=(b, i, p))                       # the NaN column counts in dbeta
    _close(ref["dbeta"], bt.grad.numpy(), "dbeta with the NaN column active")


# ------------------------------------------------------------------------------------------------ geometry
def test_restated_geometry_gives_the_library_workspace_sizes():
    dw, pair, rd = (_fn(n) for n in ("mgar_pointwise_dw_workspace_floats", "mgar_pointwise_dw_bnbwd_workspace_floats",
                                     "mgar_rowmajor_dw_workspace_floats"))
    for s in PC.DW_CASES.values():
        assert dw(s["B"], s["Cin"], s["Cout"], s["P"]) == PC.dw_geometry(s["B"], s["Cin"], s["Cout"], s["P"])["workspace"], s
    for s in PC.PAIR_CASES.values():
        assert pair(s["B"], s["Cin"], s["Cout"], s["P"]) == PC.dw_geometry(s["B"], s["Cin"], s["Cout"], s["P"], pair=True)["workspace"], s
    for s in PC.GRAD_CASES.values():
        P = s["M"] * s["ns"]
        assert dw(s["B"], s["Cp"], s["C"], P) == PC.dw_geometry(s["B"], s["Cp"], s["C"], P, grad=True)["workspace"], s
    for s in PC.RD_CASES.values():
        assert rd(s["N"], s["Co"], s["Ci"]) == PC.rd_geometry(s["N"], s["Co"], s["Ci"])["workspace"], s
    # the grid saturates: 2 048 workgroups shared among the output blocks; 256 workgroups of the row-major kernel
    for B, Cin, Cout, P in ((8, 64, 64, 1 << 20), (4, 129, 130, 1 << 18), (1, 3, 5, PC.BIG_P)):
        assert dw(B, Cin, Cout, P) == PC.dw_geometry(B, Cin, Cout, P)["workspace"]
    assert PC.dw_geometry(8, 64, 64, 1 << 20)["gx"] == 2048 and PC.dw_geometry(4, 129, 130, 1 << 18)["gx"] == 2048 // 6
    assert rd(1 << 21, 96, 128) == PC.rd_geometry(1 << 21, 96, 128)["workspace"] == 256 * 4 * 96 * 128
    assert dw(0, 4, 4, 4) == pair(1, 4, 4, 0) == rd(0, 4, 4) == 0
    big = PC.pf_geometry(1, 3, 5, PC.BIG_P)
    assert big["wgs"] == 2048 and big["tiles_per_wave"] == 2 and big["ntiles"] == PC.BIG_TILES + 1
    assert PC.pf_geometry(1, 256, 64, 132)["lds"] == 256 * 100 * 4 > 65536 >= PC.pf_geometry(1, 256, 32, 132)["lds"]


def test_every_instance_and_path_is_reached(capsys):
    table = PC.reach_table()
    with capsys.disabled():
        print()
        for what in sorted(table):
            print("  %-52s %3d  %s" % (what, len(table[what]), ", ".join(table[what][:3])))
    missing = [w for w in PC.REACH_REQUIRED if w not in table]
    assert not missing, missing
    assert "pf<2,STATS>" not in table          # Cout > 32 is refused by mgar_pointwise_conv_fwd_stats: one STATS instance exists


# ------------------------------------------------------------------------------------------------ exactness
def _exact_names(table):
    return sorted(n for n, s in table.items() if s["kind"] == "exact")


def _prologue_exact(k, x, prefix=""):
    """Every intermediate of the BatchNorm prologue, in the kernel's order, is an fp32 number."""
    if k[prefix + "mean"] is None:
        return
    C = x.shape[1]
    g = np.ones(C) if k[prefix + "gamma"] is None else k[prefix + "gamma"].astype(F64)
    b = np.zeros(C) if k[prefix + "beta"] is None else k[prefix + "beta"].astype(F64)
    sc = k[prefix + "invstd"].astype(F64) * g
    d = x.astype(F64) - k[prefix + "mean"].astype(F64).reshape(1, C, 1)
    for v in (sc, d, d * sc.reshape(1, C, 1), d * sc.reshape(1, C, 1) + b.reshape(1, C, 1), d * k[prefix + "invstd"].astype(F64).reshape(1, C, 1)):
        assert PC.roundtrips(v)


@pytest.mark.parametrize("name", _exact_names(PC.FWD_CASES))
def test_exact_forward_cases_are_exact(name):
    k = PC.fwd_case(name)
    ref = PC.fwd_ref(k)
    _prologue_exact(k, k["x"])
    assert PC.exact_margin(ref["S"], k["w"], ref["operand"]) > 1 and PC.roundtrips(ref["y"])


@pytest.mark.parametrize("name", _exact_names(PC.STATS_CASES))
def test_exact_stats_cases_are_exact_in_y(name):
    k = PC.stats_case(name)
    ref = PC.fwd_ref(k)
    _prologue_exact(k, k["x"])
    assert PC.exact_margin(ref["S"], k["w"], ref["operand"]) > 1 and PC.roundtrips(ref["y"])


@pytest.mark.parametrize("name", _exact_names(PC.DW_CASES))
def test_exact_dw_cases_are_exact(name):
    k = PC.dw_case(name)
    ref = PC.dw_ref(k)
    _prologue_exact(k, k["x"])
    assert PC.exact_margin(ref["S"], k["dy"], ref["operand"]) > 1 and PC.roundtrips(ref["dw"])


@pytest.mark.parametrize("name", _exact_names(PC.PAIR_CASES))
def test_exact_pair_cases_are_exact(name):
    k = PC.pair_case(name)
    ref = PC.pair_ref(k)
    _prologue_exact(k, k["x"])
    assert PC.exact_margin(ref["SA"], k["dy"]) > 1 and PC.exact_margin(ref["SB"], k["dy"], ref["xh"]) > 1
    g = np.ones(k["Cin"]) if k["gamma"] is None else k["gamma"].astype(F64)
    b = np.zeros(k["Cin"]) if k["beta"] is None else k["beta"].astype(F64)
    for v in (ref["A"], ref["B"], g * ref["B"], b * ref["A"], ref["dw"], ref["dgamma"], ref["dbeta"]):
        assert PC.roundtrips(v)
    assert np.abs(k["w"].astype(F64) * ref["A"]).sum(0).max() < 2.0 ** 52       # the sums over o in double


@pytest.mark.parametrize("name", _exact_names(PC.GRAD_CASES))
def test_exact_grad_cases_are_exact(name):
    k = PC.grad_case(name)
    B, C, M, ns, P = k["B"], k["C"], k["M"], k["ns"], k["P"]
    dx, A = PC.dx4_ref(k, k["coef"], k["dmask"])
    g = np.ones(C) if k["gamma"] is None else k["gamma"].astype(F64)
    inv, mu = k["invstd"].astype(F64).reshape(1, C, 1), k["mean"].astype(F64).reshape(1, C, 1)
    x3 = k["x4"].astype(F64).reshape(B, C, P)
    m0, m1 = k["coef"][:, 0].astype(F64).reshape(1, C, 1), k["coef"][:, 1].astype(F64).reshape(1, C, 1)
    d = dx * 0.0
    np.put_along_axis(d.reshape(B, C, M, ns), k["arg"].astype(np.int64)[..., None], k["dmask"].astype(F64)[..., None], -1)
    steps = (inv[0, :, 0] * g, x3 - mu, (x3 - mu) * inv, (x3 - mu) * inv * m1, d - m0, d - m0 - (x3 - mu) * inv * m1, dx)
    for v in steps:                                  # the closed form in bn_max_bwd_apply_kernel's order
        assert PC.roundtrips(v)
    _prologue_exact(k, k["x"], "in_")
    fwd, dw = PC.fwd_maxgrad_ref(k, k["coef"], k["dmask"]), PC.dw_maxgrad_ref(k, k["coef"], k["dmask"])
    assert PC.exact_margin(fwd["S"], k["w"], dx) > 1 and PC.roundtrips(fwd["y"])
    assert PC.exact_margin(dw["S"], dw["operand"], dx) > 1 and PC.roundtrips(dw["dw"])
    assert (k["dmask"][:, 3::4] == 0).all()
    assert k["arg"].max() == ns - 1 and (k["arg"] < ns).all()


@pytest.mark.parametrize("name", _exact_names(PC.RD_CASES))
def test_exact_rowmajor_cases_are_exact(name):
    k = PC.rd_case(name)
    ref = PC.rd_ref(k)
    assert PC.exact_margin(ref["S"], k["a"][:, :k["Co"]], k["f"][:, :k["Ci"]]) > 1 and PC.roundtrips(ref["dw"])


def test_quantum_and_margin():
    assert PC.quantum([3.0, 0.75, -2.5]) == 0.25 and PC.quantum([0.0]) == 1.0 and PC.quantum([8.0, 24.0]) == 8.0
    assert PC.exact_margin(np.array([2.0 ** 23]), [1.0], [0.5]) == 1.0          # 2^24 half-units: one too many


# ------------------------------------------------------------------------------------------------ the bounds hold, and bite
def _outside(got, want, bound):
    return bool((np.abs(np.asarray(got, F64) - want) > bound).any())


def _act32(x, k, relu, prefix=""):
    """The prologue in fp32, in the kernels' order: (x - mean) * (invstd * gamma) + beta, ReLU."""
    if k[prefix + "mean"] is None:
        return x.astype(F32)
    C = x.shape[1]
    g = np.ones(C, F32) if k[prefix + "gamma"] is None else k[prefix + "gamma"]
    b = np.zeros(C, F32) if k[prefix + "beta"] is None else k[prefix + "beta"]
    sc = (k[prefix + "invstd"] * g).astype(F32)
    v = ((x - k[prefix + "mean"].reshape(1, C, 1)).astype(F32) * sc.reshape(1, C, 1)).astype(F32) + b.reshape(1, C, 1)
    return np.maximum(v, F32(0)) if relu else v.astype(F32)


def _relu_off_channel(ref):
    """The channel with the most negative pre-activations, and the operand with its ReLU left out."""
    c = int((ref["pre"] < 0).sum((0, 2)).argmax())
    a = ref["operand"].copy()
    a[:, c] = ref["pre"][:, c]
    return c, a, bool((ref["pre"][:, c] < 0).any())


def _drop_masks(B, P):
    """(name, keep (B, P)): the last column of tile 0 dropped; the tail tile (the last tile of the last sample) dropped."""
    col = np.ones((B, P))
    col[0, min(PC.TILE, P) - 1] = 0.0
    tail = np.ones((B, P))
    tail[B - 1, (PC.ceil_div(P, PC.TILE) - 1) * PC.TILE:] = 0.0
    return (("last column of a tile", col), ("tail tile", tail))


@pytest.mark.parametrize("name", sorted(n for n, s in PC.FWD_CASES.items() if s["kind"] == "bounded"))
def test_forward_bound_holds_in_fp32_and_bites(name):
    k = PC.fwd_case(name)
    ref = PC.fwd_ref(k)
    y, bound = ref["y"], ref["bound"]
    a32 = _act32(k["x"], k, k["relu"])
    assert not _outside(np.einsum("oi,bip->bop", k["w"], a32), y, bound)
    for what, keep in _drop_masks(k["B"], k["P"]):
        assert _outside(y * keep[:, None, :], y, bound), what
    w = k["w"].astype(F64)
    if k["relu"] and ref["r"]:
        c, a, any_neg = _relu_off_channel(ref)
        assert any_neg and _outside(np.einsum("oi,bip->bop", w, a), y, bound), "ReLU left out in channel %d" % c
    if min(w.shape) > 1:
        assert _outside(np.einsum("oi,bip->bop", w.T.reshape(w.shape), ref["operand"]), y, bound), "W read untransposed"


@pytest.mark.parametrize("name", sorted(n for n, s in PC.STATS_CASES.items() if s["kind"] == "bounded"))
def test_stats_bound_bites(name):
    k = PC.stats_case(name)
    y = PC.fwd_ref(k)["y"].astype(F32)
    want, bound = PC.stats_ref(y)
    short = y.copy()
    short[:, :, PC.TILE - 1] = 0.0                    # the tile's last column never reached the sums
    got, _ = PC.stats_ref(short)
    assert _outside(got[:, :, 0], want[:, :, 0], bound[:, :, 0]) and _outside(got[:, :, 1], want[:, :, 1], bound[:, :, 1])
    swapped = want[:, ::-1] if want.shape[1] > 1 else None      # tile t written to slot ntiles - 1 - t
    assert swapped is None or _outside(swapped[:, :, 0], want[:, :, 0], bound[:, :, 0])


def _dw_mutants(k, ref_fn, dw, bound, B, P, geo, relu_ref):
    for what, keep in _drop_masks(B, P):
        assert _outside(ref_fn(keep=keep), dw, bound), what
    assert _outside(ref_fn(keep=PC.first_slice_columns(geo, B, P)), dw, bound), "a reduce slice lost"


@pytest.mark.parametrize("name", sorted(n for n, s in PC.DW_CASES.items() if s["kind"] == "bounded"))
def test_dw_bound_holds_in_fp32_and_bites(name):
    k = PC.dw_case(name)
    ref = PC.dw_ref(k)
    dw, bound = ref["dw"], ref["bound"]
    assert not _outside(np.einsum("bop,bip->oi", k["dy"], _act32(k["x"], k, k["relu"])), dw, bound)
    _dw_mutants(k, lambda keep: PC.dw_ref(k, keep=keep)["dw"], dw, bound, k["B"], k["P"], k["geo"], ref)
    if k["relu"] and ref["r"]:
        c, a, any_neg = _relu_off_channel(ref)
        assert any_neg and _outside(np.einsum("bop,bip->oi", k["dy"].astype(F64), a), dw, bound), "ReLU left out in channel %d" % c


@pytest.mark.parametrize("name", sorted(n for n, s in PC.PAIR_CASES.items() if s["kind"] == "bounded"))
def test_pair_bounds_bite(name):
    k = PC.pair_case(name)
    ref = PC.pair_ref(k)
    for what, keep in _drop_masks(k["B"], k["P"]) + (("a reduce slice lost", PC.first_slice_columns(k["geo"], k["B"], k["P"])),):
        mut = PC.pair_ref(k, keep=keep)
        for out, bound in (("dw", "bdw"), ("dbeta", "bbeta"), ("dgamma", "bgamma"), ("coef", "bcoef")):
            assert _outside(mut[out], ref[out], ref[bound]), (what, out)
    if k["relu"]:
        assert (ref["pre"] < 0).any()
        mut = PC.pair_ref(k, relu=0)
        for out, bound in (("dw", "bdw"), ("dbeta", "bbeta"), ("dgamma", "bgamma")):
            assert _outside(mut[out], ref[out], ref[bound]), ("ReLU left out", out)


def _grad_inputs(k):
    """coef and dmask as the device reduce would leave them, from float64 (rounded to fp32: they are inputs)."""
    B, C, M, ns, P = k["B"], k["C"], k["M"], k["ns"], k["P"]
    dmask = np.where(k["pooled"] > 0, k["dpool"], F32(0.0))
    dz = np.zeros((B, C, M, ns))
    np.put_along_axis(dz, k["arg"].astype(np.int64)[..., None], dmask.astype(F64)[..., None], -1)
    r = PC.R.bn_bwd_ref(dz.reshape(B, C, P), k["x4"].reshape(B, C, P), k["mean"], k["invstd"], k["gamma"])
    return r["coef"].astype(F32), dmask


@pytest.mark.parametrize("name", sorted(n for n, s in PC.GRAD_CASES.items() if s["kind"] == "bounded" and not s.get("fwd_only")))
def test_maxgrad_bounds_bite(name):
    k = PC.grad_case(name)
    B, C, M, ns, P = k["B"], k["C"], k["M"], k["ns"], k["P"]
    coef, dmask = _grad_inputs(k)
    assert (dmask[:, 3::4] == 0).all() and (dmask[:, 0::4] != 0).any()           # the dead channel; a live one
    fwd, dw = PC.fwd_maxgrad_ref(k, coef, dmask), PC.dw_maxgrad_ref(k, coef, dmask)
    # the closed form in fp32, in the kernels' order, through an fp32 product sum
    g = np.ones(C, F32) if k["gamma"] is None else k["gamma"]
    kk = (g * k["invstd"]).astype(F32).reshape(1, C, 1)
    d = np.zeros((B, C, M, ns), F32)
    np.put_along_axis(d, k["arg"].astype(np.int64)[..., None], dmask[..., None], -1)
    x3, d = k["x4"].reshape(B, C, P), d.reshape(B, C, P)
    t = ((x3 - k["mean"].reshape(1, C, 1)).astype(F32) * k["invstd"].reshape(1, C, 1)).astype(F32) * coef[:, 1].reshape(1, C, 1)
    dx32 = (kk * ((d - coef[:, 0].reshape(1, C, 1)).astype(F32) - t.astype(F32)).astype(F32)).astype(F32)
    assert not _outside(np.einsum("cj,bcp->bjp", k["w"], dx32), fwd["y"], fwd["bound"])
    assert not _outside(np.einsum("bcp,bjp->cj", dx32, _act32(k["x"], k, k["relu"], "in_")), dw["dw"], dw["bound"])
    # arg one slot off in the planted groups (slot 0 -> 1, ns - 1 -> ns - 2, behind the tile edge -> one further)
    for cs, m, s in k["plant"]:
        arg = k["arg"].copy()
        arg[:, cs, m] = s + 1 if s + 1 < ns else s - 1
        assert _outside(PC.fwd_maxgrad_ref(k, coef, dmask, arg=arg)["y"], fwd["y"], fwd["bound"]), ("arg shifted in group", m)
        assert _outside(PC.dw_maxgrad_ref(k, coef, dmask, arg=arg)["dw"], dw["dw"], dw["bound"]), ("arg shifted in group", m)
    assert _outside(PC.fwd_maxgrad_ref(k, coef, dmask, swap=True)["y"], fwd["y"], fwd["bound"]), "m0 and m1 swapped"
    assert _outside(PC.dw_maxgrad_ref(k, coef, dmask, swap=True)["dw"], dw["dw"], dw["bound"]), "m0 and m1 swapped"
    for what, keep in _drop_masks(B, P):
        assert _outside(fwd["y"] * keep[:, None, :], fwd["y"], fwd["bound"]), what
        assert _outside(PC.dw_maxgrad_ref(k, coef, dmask, keep=keep)["dw"], dw["dw"], dw["bound"]), what
    assert _outside(PC.dw_maxgrad_ref(k, coef, dmask, keep=PC.first_slice_columns(k["geo_dw"], B, P))["dw"], dw["dw"], dw["bound"])
    w = k["w"].astype(F64)
    if min(w.shape) > 1:
        assert _outside(np.einsum("cj,bcp->bjp", w.reshape(w.shape[::-1]).T, fwd["operand"]), fwd["y"], fwd["bound"]), "W untransposed"
    if k["relu"] and dw["r"]:
        c, a, any_neg = _relu_off_channel(dw)
        assert any_neg and _outside(np.einsum("bcp,bjp->cj", PC.dx4_ref(k, coef, dmask)[0], a), dw["dw"], dw["bound"]), "ReLU left out"


@pytest.mark.parametrize("name", sorted(n for n, s in PC.RD_CASES.items() if s["kind"] == "bounded"))
def test_rowmajor_bound_holds_in_fp32_and_bites(name):
    k = PC.rd_case(name)
    ref, geo, N = PC.rd_ref(k), k["geo"], k["N"]
    assert not _outside(k["a"][:, :k["Co"]].T @ k["f"][:, :k["Ci"]], ref["dw"], ref["bound"])
    rows = np.arange(N)
    last_of_slab = (rows != min(geo["rows"], N) - 1).astype(F64)
    tail_slab = (rows < (geo["nslab"] - 1) * geo["rows"]).astype(F64)
    slice0 = ((rows // geo["rows"]) % geo["nwaves"] >= PC.ceil_div(geo["nwaves"], PC.SLICES)).astype(F64)
    for what, keep in (("last row of a slab", last_of_slab), ("tail slab", tail_slab), ("a reduce slice lost", slice0)):
        assert _outside(PC.rd_ref(k, keep=keep)["dw"], ref["dw"], ref["bound"]), what
    wide = PC.rd_ref(dict(k, Co=k["lda"], Ci=k["ldf"]))["dw"] if k["pad"] else None      # the padding columns hold 1e30
    assert wide is None or np.abs(wide[k["Co"]:, :]).min() > 1e20
