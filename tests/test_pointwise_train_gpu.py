"""The fp32 training kernels of the shared MLPs at the op level: csrc/pointwise_fwd.hip (mgar_pointwise_conv_fwd with plain and
transposed weight strides, mgar_pointwise_conv_fwd_stats, mgar_pointwise_conv_fwd_maxgrad), csrc/pointwise_dw.hip
(mgar_pointwise_conv_dw, mgar_pointwise_conv_dw_act, mgar_pointwise_conv_dw_maxgrad, mgar_pointwise_conv_dw_bnbwd and the size
queries mgar_pointwise_dw_workspace_floats, mgar_pointwise_dw_bnbwd_workspace_floats) and csrc/rowmajor_dw.hip
(mgar_rowmajor_dw, mgar_rowmajor_dw_workspace_floats), against the float64 references of tests/pointwise_train_cases.py.
tests/test_pointwise_train_cpu.py shows, with no kernel, that those references are autograd's, that the restated launch
geometry is the library's, which instance and path every case reaches, and that every bound bites.

Calls go through `_lib` with raw pointers; dev(), nans(), guards_intact(), within() and same_bits() are those of
tests/test_query_group_gpu.py.  Every output and every workspace -- sized by the library's own query, not one float more --
starts as payload NaNs with a guard behind it that must keep its bits; guards_intact() follows every call.

  exact cases    integer / dyadic operands: the result equals float64 bit for bit (no bound appears), whatever the order of
                 the sums -- a dropped, doubled or misplaced term cannot hide;
  bounded cases  random operands, dy over four decades: |got - want64| <= gamma_u(d + r) S + 2^-149,
                 a second run bit-identical;
  folded = dense mgar_pointwise_conv_fwd_maxgrad / _dw_maxgrad against mgar_bn_act_maxpool_bwd followed by
                 mgar_pointwise_conv_fwd (W transposed) / mgar_pointwise_conv_dw_act, bit for bit: the header's promise;
  non-finite     one NaN goes exactly where autograd puts it, everything else stays exact / inside its bound."""
import numpy as np
import pytest
import torch

import pointwise_train_cases as PC
from test_query_group_gpu import GUARD, L, _fresh_guards, dev, guards_intact, nans, same_bits, within  # noqa: F401

pytestmark = pytest.mark.gpu
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
F32 = np.float32
_alive = []


@pytest.fixture(autouse=True)
def _release():
    _alive.clear()
    yield
    _alive.clear()


def hold(a):
    """dev(a) (None stays None), alive until the end of the test."""
    t = None if a is None else dev(a)
    _alive.append(t)
    return t


def ptr(t):
    return None if t is None else t.data_ptr()


def exact(what, got, want64, keep_zero_sign=False):
    """got (device fp32) equals the float64 result bit for bit.  The kernels' sums start from +0, so a zero result is +0."""
    want64 = np.asarray(want64, np.float64)
    assert PC.roundtrips(want64), "%s: the float64 result is no fp32 number -- the case is not exact" % what
    want = want64 if keep_zero_sign else want64 + 0.0
    same_bits(what, got.reshape(want.shape), torch.from_numpy(want.astype(F32)).cuda())


def nan_set(what, got, expect):
    have = torch.isnan(got).cpu().numpy().reshape(expect.shape)
    assert np.array_equal(have, expect), "%s: %d NaN where none belongs, %d missing" % (
        what, (have & ~expect).sum(), (~have & expect).sum())


def bn_ptrs(k, prefix=""):
    return tuple(ptr(hold(k[prefix + a])) for a in ("mean", "invstd", "gamma", "beta"))


def margin_holds(k, ref):
    """A ReLU case keeps every pre-activation RELU_MARGIN off zero, far outside twice the prologue's own bound."""
    if k["relu"] and ref["r"]:
        assert np.abs(ref["pre"]).min() >= 0.99 * PC.BC.RELU_MARGIN > 2.0 * ref["bpre"].max()


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(L, k, x, stats=False):
    B, Cin, Cout, P = k["B"], k["Cin"], k["Cout"], k["P"]
    wbuf, rs, cs = PC.w_buffer(k)
    y = nans(B * Cout * P)
    head = (L.fptr(x), B, Cin, P, L.fptr(hold(wbuf)), rs, cs, Cout, *bn_ptrs(k), k["relu"], L.fptr(y))
    if stats:
        st = nans(Cout * (B * P // PC.TILE) * 2)
        L.call("mgar_pointwise_conv_fwd_stats", *head, L.fptr(st), L.stream_of(x))
    else:
        st = None
        L.call("mgar_pointwise_conv_fwd", *head, L.stream_of(x))
    guards_intact()
    return y.view(B, Cout, P), (None if st is None else st.view(Cout, B * P // PC.TILE, 2))


def check_fwd(L, k, stats):
    x = hold(k["x"])
    ref = PC.fwd_ref(k)
    tag = ("fwd_stats " if stats else "fwd ") + k["name"]
    y, st = run_fwd(L, k, x, stats)
    if k["kind"] == "exact":
        exact(tag, y, ref["y"])
    else:
        margin_holds(k, ref)
        within(tag + (" wt" if k["wt"] else ""), y, ref["y"], ref["bound"])
    y2, st2 = run_fwd(L, k, x, stats)
    same_bits(tag + " second run", y2, y)
    if stats:
        want, bound = PC.stats_ref(y.cpu().numpy())
        within(tag + " tile mean", st[:, :, 0], want[:, :, 0], bound[:, :, 0])
        within(tag + " tile M2", st[:, :, 1], want[:, :, 1], bound[:, :, 1])
        same_bits(tag + " tiles second run", st2, st)
        plain, _ = run_fwd(L, k, x, False)
        same_bits(tag + " y of the plain entry", plain, y)


@pytest.mark.parametrize("name", sorted(PC.FWD_CASES))
def test_pointwise_conv_fwd(L, name):
    check_fwd(L, PC.fwd_case(name), False)


@pytest.mark.parametrize("name", sorted(PC.STATS_CASES))
def test_pointwise_conv_fwd_stats(L, name):
    check_fwd(L, PC.stats_case(name), True)


@pytest.mark.parametrize("name", sorted(PC.FWD_REFUSED))
def test_pointwise_conv_fwd_refuses_and_writes_nothing(L, name):
    B, Cin, Cout, P = PC.FWD_REFUSED[name]
    x, w, one = hold(np.ones(max(B * Cin * P, 1), F32)), hold(np.ones(max(Cout * Cin, 1), F32)), hold(np.ones(max(Cin, 1), F32))
    y, st = nans(B * Cout * P), nans(2 * Cout * max(B * P // PC.TILE, 1))
    head = (L.fptr(x), B, Cin, P, L.fptr(w), Cin, 1, Cout, L.fptr(one), L.fptr(one), None, None, 1, L.fptr(y))
    assert L.raw("mgar_pointwise_conv_fwd", *head, L.stream_of(x)) == EUNSUPPORTED
    if P % PC.TILE == 0 and Cout <= 32:
        assert L.raw("mgar_pointwise_conv_fwd_stats", *head, L.fptr(st), L.stream_of(x)) == EUNSUPPORTED
    guards_intact()
    assert torch.isnan(y).all() and torch.isnan(st).all()


def test_pointwise_conv_fwd_stats_refuses_what_its_instance_cannot_hold(L):
    x, w, y, st = hold(np.ones(33 * 256, F32)), hold(np.ones(33 * 4, F32)), nans(33 * 256), nans(33 * 4)
    head = lambda Cout, P: (L.fptr(x), 1, 4, P, L.fptr(w), 4, 1, Cout, None, None, None, None, 0, L.fptr(y))  # noqa: E731
    assert L.raw("mgar_pointwise_conv_fwd_stats", *head(33, 128), L.fptr(st), L.stream_of(x)) == EUNSUPPORTED
    assert L.raw("mgar_pointwise_conv_fwd_stats", *head(4, 132), L.fptr(st), L.stream_of(x)) == EINVAL      # P % 128 != 0
    assert L.raw("mgar_pointwise_conv_fwd_stats", *head(4, 128), None, L.stream_of(x)) == EINVAL
    guards_intact()
    assert torch.isnan(y).all() and torch.isnan(st).all()


def test_forward_entries_write_nothing_for_an_empty_input(L):
    x, w, y, st = hold(np.ones(64, F32)), hold(np.ones(64, F32)), nans(64), nans(64)
    u8 = torch.zeros(64 + GUARD, dtype=torch.uint8, device="cuda")
    for B, P in ((0, 128), (2, 0)):
        head = (L.fptr(x), B, 4, P, L.fptr(w), 4, 1, 4, None, None, None, None, 0, L.fptr(y))
        assert L.raw("mgar_pointwise_conv_fwd", *head, L.stream_of(x)) == OK
        assert L.raw("mgar_pointwise_conv_fwd_stats", *head, L.fptr(st), L.stream_of(x)) == OK
    for B, M in ((0, 4), (2, 0)):
        assert L.raw("mgar_pointwise_conv_fwd_maxgrad", L.fptr(x), B, 4, M, 4, L.fptr(w), 1, 4, 4, L.fptr(x), L.fptr(x), None,
                     L.fptr(x), u8.data_ptr(), L.fptr(x), L.fptr(y), L.stream_of(x)) == OK
    guards_intact()
    assert torch.isnan(y).all() and torch.isnan(st).all()


# ------------------------------------------------------------------------------------------------ dW, plain and _act
def run_dw(L, k, x, dy):
    B, Cin, Cout, P = k["B"], k["Cin"], k["Cout"], k["P"]
    n = L.raw("mgar_pointwise_dw_workspace_floats", B, Cin, Cout, P)
    assert n == k["geo"]["workspace"]
    ws, dw = nans(n), nans(Cout * Cin)
    if k["act"] is None:
        L.call("mgar_pointwise_conv_dw", L.fptr(x), L.fptr(dy), B, Cin, Cout, P, L.fptr(ws), L.fptr(dw), L.stream_of(x))
    else:
        L.call("mgar_pointwise_conv_dw_act", L.fptr(x), L.fptr(dy), B, Cin, Cout, P, *bn_ptrs(k), k["relu"], L.fptr(ws), L.fptr(dw),
               L.stream_of(x))
    guards_intact()
    return dw.view(Cout, Cin)


@pytest.mark.parametrize("name", sorted(PC.DW_CASES))
def test_pointwise_conv_dw_and_dw_act(L, name):
    k = PC.dw_case(name)
    x, dy = hold(k["x"]), hold(k["dy"])
    ref = PC.dw_ref(k)
    dw = run_dw(L, k, x, dy)
    if k["kind"] == "exact":
        exact("dw " + name, dw, ref["dw"])
    else:
        margin_holds(k, ref)
        within("dw%s %s" % ("" if k["act"] is None else "_act", name), dw, ref["dw"], ref["bound"])
    same_bits("dw %s second run" % name, run_dw(L, k, x, dy), dw)
    if k["act"] is None:     # both entries, whichever ran above
        B, Cin, Cout, P = k["B"], k["Cin"], k["Cout"], k["P"]
        for entry, extra in (("mgar_pointwise_conv_dw", ()), ("mgar_pointwise_conv_dw_act", (None, None, None, None, 0))):
            ws, other = nans(k["geo"]["workspace"]), nans(Cout * Cin)
            L.call(entry, L.fptr(x), L.fptr(dy), B, Cin, Cout, P, *extra, L.fptr(ws), L.fptr(other), L.stream_of(x))
            guards_intact()
            same_bits("dw %s %s" % (name, entry), other.view(Cout, Cin), dw)


def test_dw_entries_zero_fill_for_an_empty_input_and_refuse_what_they_cannot_hold(L):
    x, ws = hold(np.ones(4096, F32)), nans(4096)
    u8 = torch.zeros(64 + GUARD, dtype=torch.uint8, device="cuda")
    st = L.stream_of(x)
    for B, P in ((0, 128), (2, 0)):
        a, b, c = nans(12), nans(12), nans(12)
        assert L.raw("mgar_pointwise_conv_dw", L.fptr(x), L.fptr(x), B, 3, 4, P, L.fptr(ws), L.fptr(a), st) == OK
        assert L.raw("mgar_pointwise_conv_dw_act", L.fptr(x), L.fptr(x), B, 3, 4, P, L.fptr(x), L.fptr(x), None, None, 1, L.fptr(ws),
                     L.fptr(b), st) == OK
        assert L.raw("mgar_pointwise_conv_dw_maxgrad", L.fptr(x), L.fptr(x), B, 3, 4, P // 4, 4, None, None, None, None, 0, L.fptr(x),
                     L.fptr(x), None, L.fptr(x), u8.data_ptr(), L.fptr(x), L.fptr(ws), L.fptr(c), st) == OK
        guards_intact()
        for t in (a, b, c):
            assert (t == 0).all()
        coef, d = nans(6), nans(12)
        assert L.raw("mgar_pointwise_conv_dw_bnbwd", L.fptr(x), L.fptr(x), L.fptr(x), B, 3, 4, P, L.fptr(x), L.fptr(x), None, None, 1,
                     L.fptr(ws), L.fptr(d), None, None, L.fptr(coef), st) == EINVAL
        assert L.raw("mgar_pointwise_dw_workspace_floats", B, 3, 4, P) == 0
        assert L.raw("mgar_pointwise_dw_bnbwd_workspace_floats", B, 3, 4, P) == 0
    out, coef = nans(65 * 65), nans(130)
    for name, (B, Cin, Cout, P) in PC.PAIR_REFUSED.items():
        assert L.raw("mgar_pointwise_conv_dw_bnbwd", L.fptr(x), L.fptr(x), L.fptr(x), B, Cin, Cout, P, L.fptr(x), L.fptr(x), None, None,
                     1, L.fptr(ws), L.fptr(out), None, None, L.fptr(coef), st) == EUNSUPPORTED, name
    for name, r in PC.GRAD_REFUSED.items():
        assert L.raw("mgar_pointwise_conv_dw_maxgrad", L.fptr(x), L.fptr(x), 1, r["Cp"], r["C"], 2, r["ns"], None, None, None, None, 0,
                     L.fptr(x), L.fptr(x), None, L.fptr(x), u8.data_ptr(), L.fptr(x), L.fptr(ws), L.fptr(out), st) == EUNSUPPORTED, name
        assert L.raw("mgar_pointwise_conv_fwd_maxgrad", L.fptr(x), 1, r["C"], 2, r["ns"], L.fptr(x), 1, r["Cp"], r["Cp"], L.fptr(x),
                     L.fptr(x), None, L.fptr(x), u8.data_ptr(), L.fptr(x), L.fptr(out), st) == EUNSUPPORTED, name
    guards_intact()
    assert torch.isnan(out).all() and torch.isnan(coef).all() and torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------ pair mode
def run_pair(L, k, x, dy, skip=()):
    B, Cin, Cout, P = k["B"], k["Cin"], k["Cout"], k["P"]
    n = L.raw("mgar_pointwise_dw_bnbwd_workspace_floats", B, Cin, Cout, P)
    assert n == k["geo"]["workspace"]
    ws = nans(n)
    out = dict(dw=nans(Cout * Cin), dgamma=nans(Cin), dbeta=nans(Cin), coef=nans(2 * Cin))
    p = {a: (None if a in skip else L.fptr(t)) for a, t in out.items()}
    mean, invstd, gamma, beta = bn_ptrs(k)
    L.call("mgar_pointwise_conv_dw_bnbwd", L.fptr(x), L.fptr(dy), L.fptr(hold(k["w"])), B, Cin, Cout, P, mean, invstd, gamma, beta,
           k["relu"], L.fptr(ws), p["dw"], p["dgamma"], p["dbeta"], p["coef"], L.stream_of(x))
    guards_intact()
    out["dw"], out["coef"] = out["dw"].view(Cout, Cin), out["coef"].view(Cin, 2)
    return out


PAIR_OUT = (("dw", "bdw"), ("dgamma", "bgamma"), ("dbeta", "bbeta"), ("coef", "bcoef"))


@pytest.mark.parametrize("name", sorted(PC.PAIR_CASES))
def test_pointwise_conv_dw_bnbwd(L, name):
    k = PC.pair_case(name)
    x, dy = hold(k["x"]), hold(k["dy"])
    ref = PC.pair_ref(k)
    got = run_pair(L, k, x, dy)
    if k["kind"] == "exact":
        for what in ("dw", "dgamma", "dbeta"):
            exact("dw_bnbwd %s %s" % (name, what), got[what], ref[what], keep_zero_sign=what == "dw")
        n = np.float64(k["B"] * k["P"])          # coef = (float)(sum / n): the same division in double, rounded once
        same_bits("dw_bnbwd %s coef" % name, got["coef"],
                  torch.from_numpy((np.stack([ref["dbeta"], ref["dgamma"]], 1) / n + 0.0).astype(F32)).cuda())
    else:
        if k["relu"]:
            assert np.abs(ref["pre"]).min() >= 0.99 * PC.BC.RELU_MARGIN > 2.0 * ref["bpre"].max()
        for what, bound in PAIR_OUT:
            within("dw_bnbwd %s %s" % (name, what), got[what], ref[what], ref[bound])
    again = run_pair(L, k, x, dy)
    for what, _ in PAIR_OUT:
        same_bits("dw_bnbwd %s %s second run" % (name, what), again[what], got[what])


@pytest.mark.parametrize("skip", ["dw", "dgamma", "dbeta"])
def test_pointwise_conv_dw_bnbwd_optional_outputs(L, skip):
    """dw, dgamma, dbeta NULL in turn: the buffer the call was not given keeps its NaNs, the other outputs keep their bits."""
    k = PC.pair_case("b_ci17_co33_b3_p131")
    x, dy = hold(k["x"]), hold(k["dy"])
    full, part = run_pair(L, k, x, dy), run_pair(L, k, x, dy, skip=(skip,))
    assert torch.isnan(part[skip]).all()
    for what, _ in PAIR_OUT:
        if what != skip:
            same_bits("dw_bnbwd without %s: %s" % (skip, what), part[what], full[what])


# ------------------------------------------------------------------------------------------------ GRAD operand mode
def grad_state(L, k):
    """Device inputs of a GRAD case; a bounded one gets coef and dmask from mgar_bn_act_maxpool_bwd_reduce and the dense dx4
    from mgar_bn_act_maxpool_bwd on the same forward state (pooled, arg, xarg)."""
    B, C, M, ns, P = k["B"], k["C"], k["M"], k["ns"], k["P"]
    s = dict(x4=hold(k["x4"]), x=hold(k["x"]), w=hold(k["w"]), mean=hold(k["mean"]), invstd=hold(k["invstd"]), gamma=hold(k["gamma"]),
             arg=hold(k["arg"]))
    if k["kind"] == "exact":
        s.update(coef=hold(k["coef"]), dmask=hold(k["dmask"]), dx4=None)
        return s
    pooled, xarg, dpool = hold(k["pooled"]), hold(k["xarg"]), hold(k["dpool"])
    nws = L.raw("mgar_bn_workspace_floats", B, C, P)
    ws, dgamma, dbeta, coef, dmask = nans(nws), nans(C), nans(C), nans(2 * C), nans(B * C * M)
    L.call("mgar_bn_act_maxpool_bwd_reduce", L.fptr(dpool), 0, -1, 0, L.fptr(pooled), ptr(s["arg"]), L.fptr(s["x4"]), L.fptr(xarg), B, C,
           M, ns, L.fptr(s["mean"]), L.fptr(s["invstd"]), 1, L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(coef), L.fptr(dmask),
           L.stream_of(dpool))
    guards_intact()
    ws2, dg2, db2, dx4 = nans(nws), nans(C), nans(C), nans(B * C * P)
    L.call("mgar_bn_act_maxpool_bwd", L.fptr(dpool), L.fptr(pooled), ptr(s["arg"]), L.fptr(s["x4"]), L.fptr(xarg), B, C, M, ns,
           L.fptr(s["mean"]), L.fptr(s["invstd"]), ptr(s["gamma"]), 1, L.fptr(ws2), L.fptr(dg2), L.fptr(db2), L.fptr(dx4), L.stream_of(dpool))
    guards_intact()
    want_mask = np.where(k["pooled"] > 0, k["dpool"], F32(0.0))
    same_bits("grad %s dmask" % k["name"], dmask.view(B, C, M), torch.from_numpy(want_mask).cuda())
    s.update(coef=coef, dmask=dmask, dx4=dx4)
    return s


def run_fwd_maxgrad(L, k, s):
    B, C, Cp, M, ns, P = k["B"], k["C"], k["Cp"], k["M"], k["ns"], k["P"]
    y = nans(B * Cp * P)
    L.call("mgar_pointwise_conv_fwd_maxgrad", L.fptr(s["x4"]), B, C, M, ns, L.fptr(s["w"]), 1, Cp, Cp, L.fptr(s["mean"]),
           L.fptr(s["invstd"]), ptr(s["gamma"]), L.fptr(s["coef"]), ptr(s["arg"]), L.fptr(s["dmask"]), L.fptr(y), L.stream_of(y))
    guards_intact()
    return y.view(B, Cp, P)


def run_dw_maxgrad(L, k, s):
    B, C, Cp, M, ns, P = k["B"], k["C"], k["Cp"], k["M"], k["ns"], k["P"]
    n = L.raw("mgar_pointwise_dw_workspace_floats", B, Cp, C, P)
    assert n == k["geo_dw"]["workspace"]
    ws, dw = nans(n), nans(C * Cp)
    L.call("mgar_pointwise_conv_dw_maxgrad", L.fptr(s["x"]), L.fptr(s["x4"]), B, Cp, C, M, ns, *bn_ptrs(k, "in_"), k["relu"],
           L.fptr(s["mean"]), L.fptr(s["invstd"]), ptr(s["gamma"]), L.fptr(s["coef"]), ptr(s["arg"]), L.fptr(s["dmask"]), L.fptr(ws),
           L.fptr(dw), L.stream_of(dw))
    guards_intact()
    return dw.view(C, Cp)


@pytest.mark.parametrize("name", sorted(PC.GRAD_CASES))
def test_maxgrad_entries_against_float64_and_the_dense_route(L, name):
    k = PC.grad_case(name)
    B, C, Cp, P = k["B"], k["C"], k["Cp"], k["P"]
    s = grad_state(L, k)
    coef, dmask = s["coef"].cpu().numpy(), s["dmask"].cpu().numpy()
    y = run_fwd_maxgrad(L, k, s)
    ref = PC.fwd_maxgrad_ref(k, coef, dmask)
    if k["kind"] == "exact":
        exact("fwd_maxgrad " + name, y, ref["y"])
    else:
        within("fwd_maxgrad " + name, y, ref["y"], ref["bound"])
        dense = nans(B * Cp * P)
        L.call("mgar_pointwise_conv_fwd", L.fptr(s["dx4"]), B, C, P, L.fptr(s["w"]), 1, Cp, Cp, None, None, None, None, 0, L.fptr(dense),
               L.stream_of(dense))
        guards_intact()
        same_bits("fwd_maxgrad %s against the dense route" % name, y, dense.view(B, Cp, P))
    same_bits("fwd_maxgrad %s second run" % name, run_fwd_maxgrad(L, k, s), y)
    if k.get("fwd_only"):
        return
    dw = run_dw_maxgrad(L, k, s)
    ref = PC.dw_maxgrad_ref(k, coef, dmask)
    if k["kind"] == "exact":
        exact("dw_maxgrad " + name, dw, ref["dw"])
    else:
        margin_holds(k, ref)
        within("dw_maxgrad " + name, dw, ref["dw"], ref["bound"])
        ws, dense = nans(k["geo_dw"]["workspace"]), nans(C * Cp)
        L.call("mgar_pointwise_conv_dw_act", L.fptr(s["x"]), L.fptr(s["dx4"]), B, Cp, C, P, *bn_ptrs(k, "in_"), k["relu"], L.fptr(ws),
               L.fptr(dense), L.stream_of(dense))
        guards_intact()
        same_bits("dw_maxgrad %s against the dense route" % name, dw, dense.view(C, Cp))
    same_bits("dw_maxgrad %s second run" % name, run_dw_maxgrad(L, k, s), dw)


# ------------------------------------------------------------------------------------------------ rowmajor_dw
def run_rd(L, k, a, f):
    N, Co, Ci = k["N"], k["Co"], k["Ci"]
    n = L.raw("mgar_rowmajor_dw_workspace_floats", N, Co, Ci)
    assert n == k["geo"]["workspace"]
    ws, dw = nans(n), nans(Co * Ci)
    L.call("mgar_rowmajor_dw", L.fptr(a), k["lda"], L.fptr(f), k["ldf"], N, Co, Ci, L.fptr(ws), L.fptr(dw), L.stream_of(a))
    guards_intact()
    return dw.view(Co, Ci)


@pytest.mark.parametrize("name", sorted(PC.RD_CASES))
def test_rowmajor_dw(L, name):
    k = PC.rd_case(name)
    a, f = hold(k["a"]), hold(k["f"])
    ref = PC.rd_ref(k)
    dw = run_rd(L, k, a, f)
    if k["kind"] == "exact":
        exact("rowmajor_dw " + name, dw, ref["dw"])
    else:
        within("rowmajor_dw " + name, dw, ref["dw"], ref["bound"])
    same_bits("rowmajor_dw %s second run" % name, run_rd(L, k, a, f), dw)


def test_rowmajor_dw_refusals_and_empty_input(L):
    a, ws, dw = hold(np.ones(4096, F32)), nans(4 * 97 * 129), nans(97 * 129)
    st = L.stream_of(a)
    for name, (Co, Ci, code) in PC.RD_REFUSED.items():
        assert L.raw("mgar_rowmajor_dw", L.fptr(a), Co, L.fptr(a), Ci, 8, Co, Ci, L.fptr(ws), L.fptr(dw), st) == code, name
    assert L.raw("mgar_rowmajor_dw", L.fptr(a), 32, L.fptr(a), 5, 8, 33, 5, L.fptr(ws), L.fptr(dw), st) == EINVAL     # lda < Co
    assert L.raw("mgar_rowmajor_dw", L.fptr(a), 33, L.fptr(a), 4, 8, 33, 5, L.fptr(ws), L.fptr(dw), st) == EINVAL     # ldf < Ci
    guards_intact()
    assert torch.isnan(dw).all() and torch.isnan(ws).all()
    assert L.raw("mgar_rowmajor_dw_workspace_floats", 0, 33, 5) == 0
    out = nans(33 * 5)
    assert L.raw("mgar_rowmajor_dw", None, 33, None, 5, 0, 33, 5, None, L.fptr(out), st) == OK
    guards_intact()
    assert (out == 0).all()


# ------------------------------------------------------------------------------------------------ NaN
def test_a_nan_in_the_maxgrad_operands_goes_where_autograd_puts_it(L):
    """Exact case x_ns12_m11 (groups straddle tiles).  A NaN at x4[b, c, m, s] is the NaN of dx4[b, c, m * ns + s]: that
    column of sample b in every row of dX, row c of dW.  A NaN at dmask[b, c, m] sits at the group's arg column only.  A NaN
    in x behind its BatchNorm + ReLU is column j of dW.  Everything else keeps the float64 bits."""
    k = dict(PC.grad_case("x_ns12_m11"))
    B, C, Cp, M, ns, P = k["B"], k["C"], k["Cp"], k["M"], k["ns"], k["P"]
    clean = (PC.fwd_maxgrad_ref(k, k["coef"], k["dmask"]), PC.dw_maxgrad_ref(k, k["coef"], k["dmask"]))
    x4, dmask, x = k["x4"].copy(), k["dmask"].copy(), k["x"].copy()
    b1, c1, m1, s1 = 0, 4, 10, 9                    # behind the tile edge of a straddling group
    b2, c2, m2 = 2, 8, 3
    assert c2 % 4 != 3
    x4[b1, c1, m1, s1] = np.nan
    dmask[b2, c2, m2] = np.nan
    k.update(x4=x4, dmask=dmask)
    s = grad_state(L, k)
    y = run_fwd_maxgrad(L, k, s)
    expect = np.zeros((B, Cp, P), bool)
    expect[b1, :, m1 * ns + s1] = True
    expect[b2, :, m2 * ns + int(k["arg"][b2, c2, m2])] = True
    nan_set("fwd_maxgrad", y, expect)
    got, want = y.cpu().numpy()[~expect], (clean[0]["y"] + 0.0).astype(F32)[~expect]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "fwd_maxgrad: a clean column lost its bits"
    j, bj, pj = 5, 1, 77
    x[bj, j, pj] = np.nan
    k.update(x=x)
    s = grad_state(L, k)
    dw = run_dw_maxgrad(L, k, s)
    expect = np.zeros((C, Cp), bool)
    expect[[c1, c2], :] = True
    expect[:, j] = True
    nan_set("dw_maxgrad", dw, expect)
    got, want = dw.cpu().numpy()[~expect], (clean[1]["dw"] + 0.0).astype(F32)[~expect]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "dw_maxgrad: a clean cell lost its bits"


@pytest.mark.parametrize("name", ["b_ci17_co33_b3_p131", "b_ci32_co33_b3_p260"], ids=["scalar_staging", "vector_staging"])
def test_a_nan_activation_in_dw_bnbwd_reaches_dw_and_dgamma_as_autograd(L, name):
    """in_relu = 1 and one NaN in x[., i, .]: float64 autograd through BatchNorm -> ReLU -> conv gives dW[:, i] and dgamma[i]
    NaN and dbeta[i] finite (tests/test_pointwise_train_cpu.py); coef follows dgamma / dbeta.  The NaN column counts as active
    in dbeta.  Every other output stays inside its bound."""
    k = dict(PC.pair_case(name))
    assert k["relu"] == 1
    B, Cin, Cout, P = k["B"], k["Cin"], k["Cout"], k["P"]
    b, i, p = B - 1, 5, P - 3
    ref = PC.pair_ref(k, force_on=(b, i, p))
    x = k["x"].copy()
    x[b, i, p] = np.nan
    got = run_pair(L, k, hold(x), hold(k["dy"]))
    e_dw, e_vec, e_coef = np.zeros((Cout, Cin), bool), np.zeros(Cin, bool), np.zeros((Cin, 2), bool)
    e_dw[:, i], e_vec[i], e_coef[i, 1] = True, True, True
    nan_set("dw_bnbwd dw", got["dw"], e_dw)
    nan_set("dw_bnbwd dgamma", got["dgamma"], e_vec)
    nan_set("dw_bnbwd dbeta", got["dbeta"], np.zeros(Cin, bool))
    nan_set("dw_bnbwd coef", got["coef"], e_coef)
    ok = np.arange(Cin) != i
    got = {what: t.cpu().numpy() for what, t in got.items()}
    within("dw_bnbwd nan %s dw" % name, got["dw"][:, ok], ref["dw"][:, ok], ref["bdw"][:, ok])
    within("dw_bnbwd nan %s dgamma" % name, got["dgamma"][ok], ref["dgamma"][ok], ref["bgamma"][ok])
    within("dw_bnbwd nan %s dbeta" % name, got["dbeta"], ref["dbeta"], ref["bbeta"])
    within("dw_bnbwd nan %s coef0" % name, got["coef"][:, 0], ref["coef"][:, 0], ref["bcoef"][:, 0])


# ------------------------------------------------------------------------------------------------ coverage of the header
ENTRIES = ("mgar_pointwise_conv_fwd", "mgar_pointwise_conv_fwd_stats", "mgar_pointwise_conv_fwd_maxgrad", "mgar_pointwise_conv_dw",
           "mgar_pointwise_conv_dw_act", "mgar_pointwise_conv_dw_maxgrad", "mgar_pointwise_conv_dw_bnbwd",
           "mgar_pointwise_dw_workspace_floats", "mgar_pointwise_dw_bnbwd_workspace_floats", "mgar_rowmajor_dw",
           "mgar_rowmajor_dw_workspace_floats")
# eval-mode and bf16 point-wise entries: tests/test_mlp_eval_gpu.py, test_pointwise_bf16_gpu.py, test_pointwise_wide_bf16_gpu.py
ELSEWHERE = ("mgar_pointwise_conv_maxpool_eval", "mgar_pointwise_conv_fwd_bf16", "mgar_pointwise_mfma", "mgar_pointwise_wide")


def test_every_training_entry_point_of_the_family_is_called_here():
    import re
    from multimodal_gar_amd import _lib
    src = open(__file__).read()
    family = [n for n in _lib._protos if n.startswith(("mgar_pointwise_", "mgar_rowmajor_")) and not n.startswith(ELSEWHERE)]
    assert sorted(family) == sorted(ENTRIES), sorted(set(family) ^ set(ENTRIES))
    for n in ENTRIES:
        assert re.search(r'(call|raw)\(\s*"%s"' % n, src), "%s is never called in this file" % n
