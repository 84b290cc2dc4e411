"""Query-and-group (csrc/query_group.hip): every C entry point outside the inverse-index route against the float64
references of torch_refs.py, on the hand-built inputs of query_group_cases.py (tests/test_query_group_cpu.py shows,
with no kernel, that the references are the reference's op chain and that every bound below is satisfiable).

The entry points are called through `_lib`, so strides and pointer offsets are the test's.  Every output starts as a
NaN with a payload of its own and has GUARD more such elements behind it, which must keep their bits: a kernel that
writes past its last channel or column is caught whatever it writes.  The accumulate-into targets start as zeros
with a zero guard behind them.  Every input has GUARD finite elements of slack behind it, so that a kernel that
over-runs reads defined memory.  The bounds are rounding counts (torch_refs.qg_*_bound, derivations in DESIGN.md
section 5b), none is fitted to what a kernel returned:

  plain forward   y is the source element, rel the fp32 subtraction: torch.equal against the fp32 chain;
  proj forward    |y - ref| <= 6 u (|zf| + sum |wx_i| |rel_i|) + 2^-149;
  bf16 twins      the fp32 kernel's output (on the bf16 inputs) rounded to bf16, bit for bit;
  LDS backward    the fixed-point bound of qg_batch_bwd_lds_kernel, two runs and both entry points bit-equal;
  atomic backward |err| <= (k - 1) u sum|g| + spacing(fp32(want)) per cell; unreferenced cells exactly 0;
  tile statistics mean / M2 partials and the finalised mean / invstd against float64 of the fp32 y the kernel wrote
                  (itself pinned elementwise by the proj bound), from the kernel's summation shape.

`record_error` logs for each comparison the share of its bound that was used."""
import numpy as np
import pytest
import torch

import query_group_cases as QC
import torch_refs as R
from conftest import record_error

pytestmark = pytest.mark.gpu
GUARD = 16384                      # >= QG_CCHUNK channels of the widest batch case (8 x 1 875 columns)
NAN_BITS = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.bfloat16: (torch.int16, 0x7FC1)}
BF16 = torch.bfloat16
_guarded = []                      # (whole buffer, elements in front of the guard) of every nans() of the running test


@pytest.fixture(scope="module")
def L():
    from multimodal_gar_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _fresh_guards():
    _guarded.clear()
    yield
    _guarded.clear()


def dev(a):
    """The array on the device, with GUARD elements of finite slack behind it."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((a.numel() + GUARD,), 1e30 if a.is_floating_point() else 0, dtype=a.dtype, device="cuda")
    buf[:a.numel()] = a.reshape(-1).cuda()
    return buf[:a.numel()].view(a.shape)


def nans(numel, dtype=torch.float32):
    """An output buffer of payload NaNs (at least one element, so that its pointer is never NULL) with GUARD more
    behind it; guards_intact() checks those."""
    numel = max(int(numel), 1)
    as_int, bits = NAN_BITS[dtype]
    buf = torch.full((numel + GUARD,), bits, dtype=as_int, device="cuda").view(dtype)
    _guarded.append((buf, numel))
    return buf[:numel]


def guards_intact():
    torch.cuda.synchronize()
    for i, (buf, numel) in enumerate(_guarded):
        as_int, bits = NAN_BITS[buf.dtype]
        touched = int((buf.view(as_int)[numel:] != bits).sum())
        assert touched == 0, "output buffer %d (%d elements): %d elements written behind it" % (i, numel, touched)


def _f64(a):
    return a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)


def within(what, got, want, bound):
    """|got - want| <= bound elementwise; logs the largest err / bound (where the bound is 0, equality is demanded)."""
    got, want = _f64(got), _f64(want)
    bound = np.broadcast_to(_f64(bound), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err = np.abs(got - want)
    pos = bound > 0
    used = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print("%s: worst err / bound %.3g (max err %.3g)" % (what, used, err.max() if err.size else 0.0))
    record_error(what, used, 1.0, 1.0)
    bad = err > bound
    assert not bad.any(), "%s: %d cells outside the bound, worst err %g at bound %g" % (
        what, bad.sum(), err[bad].max(), bound[bad][np.argmax(err[bad])])


def same_bits(what, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    as_int = NAN_BITS[got.dtype][0]
    ok = torch.equal(got.contiguous().view(as_int), want.contiguous().view(as_int))
    record_error(what, 0.0 if ok else 1.0, 1.0, 0.0)
    assert ok, "%s: not bit-equal" % what


# ------------------------------------------------------------------------------------------------ batch forward
def _batch_chain_fp32(k):
    """The op chain in fp32 numpy: gather, subtract the centre (one fp32 rounding), gather the features."""
    bi = np.arange(k["b"])[:, None, None]
    rel = (k["xyz"][bi, k["idx"]] - k["new_xyz"][:, :, None, :]).transpose(0, 3, 1, 2)
    flat = np.broadcast_to(k["idx"].reshape(k["b"], 1, -1), (k["b"], k["c"], k["m"] * k["ns"]))
    feat = np.take_along_axis(k["feats"], flat, axis=2).reshape(k["b"], k["c"], k["m"], k["ns"])
    return np.ascontiguousarray(rel), np.ascontiguousarray(feat)


@pytest.mark.parametrize("name", sorted(QC.BATCH_FWD_CASES))
def test_batch_forward_plain_proj_and_bf16(L, name):
    k = QC.batch_fwd_case(name)
    b, c, m, ns, n = k["b"], k["c"], k["m"], k["ns"], k["n"]
    cols = m * ns
    xyz, new_xyz, idx, feats, wx = (dev(k[key]) for key in ("xyz", "new_xyz", "idx", "feats", "wx"))
    st = L.stream_of(xyz)
    sizes = (b, c, n, m, ns)
    geo = (L.fptr(xyz), L.fptr(new_xyz))
    rel32, feat32 = _batch_chain_fp32(k)
    chain = dev(np.concatenate([rel32, feat32], 1))
    # plain
    out = nans(b * (3 + c) * cols)
    L.call("mgar_query_group_batch_fwd", *sizes, *geo, L.fptr(feats) if c else None, L.iptr(idx), L.fptr(out), st)
    # proj, with and without rel_out
    zf = feats if c else nans(1)
    wxp = wx if c else nans(1)
    rel_out, y_out, y_only = nans(b * 3 * cols), nans(b * c * cols), nans(b * c * cols)
    L.call("mgar_query_group_proj_batch_fwd", *sizes, *geo, L.fptr(zf), L.fptr(wxp), L.iptr(idx),
           L.fptr(rel_out), L.fptr(y_out), st)
    L.call("mgar_query_group_proj_batch_fwd", *sizes, *geo, L.fptr(zf), L.fptr(wxp), L.iptr(idx),
           None, L.fptr(y_only), st)
    # bf16 twins, and the fp32 kernels on the bf16-rounded payload
    fb = dev(feats.bfloat16().cpu().view(torch.int16).numpy()).view(BF16)
    fb32 = dev(fb.float().cpu().numpy())
    out32, outb = nans(b * (3 + c) * cols), nans(b * (3 + c) * cols, BF16)
    L.call("mgar_query_group_batch_fwd", *sizes, *geo, L.fptr(fb32) if c else None, L.iptr(idx), L.fptr(out32), st)
    L.call("mgar_query_group_batch_fwd_bf16", *sizes, *geo, L.pptr(fb, BF16) if c else None, L.iptr(idx),
           L.pptr(outb, BF16), st)
    if c:
        rel_b, y_b, y32 = nans(b * 3 * cols, BF16), nans(b * c * cols, BF16), nans(b * c * cols)
        L.call("mgar_query_group_proj_batch_fwd", *sizes, *geo, L.fptr(fb32), L.fptr(wx), L.iptr(idx),
               None, L.fptr(y32), st)
        L.call("mgar_query_group_proj_batch_fwd_bf16", *sizes, *geo, L.pptr(fb, BF16), L.fptr(wx), L.iptr(idx),
               L.pptr(rel_b, BF16), L.pptr(y_b, BF16), st)
    guards_intact()                                            # nothing behind any output, whatever c % QG_CCHUNK is
    # plain: exact
    same_bits("plain batch fwd", out.view(b, 3 + c, m, ns), chain)
    # proj: bounded; rel exact; rel_out = NULL gives the same y
    rel64, y64 = R.query_group_batch_ref(k["xyz"], k["new_xyz"], k["feats"], k["idx"], k["wx"])
    bound = R.qg_proj_fwd_bound(torch.from_numpy(feat32), k["wx"], rel64)
    same_bits("proj batch fwd rel", rel_out.view(b, 3, m, ns), dev(rel32))
    if c:
        within("proj batch fwd y", y_out.view(b, c, m, ns), y64, bound)
        same_bits("proj batch fwd y without rel_out", y_only, y_out)
    else:
        assert torch.isnan(y_out).all() and torch.isnan(y_only).all()          # c = 0: nothing to write
    same_bits("plain batch fwd bf16", outb, out32.bfloat16())
    if c:
        same_bits("proj batch fwd bf16 y", y_b, y32.bfloat16())
        same_bits("proj batch fwd bf16 rel", rel_b, rel_out.bfloat16())


# ------------------------------------------------------------------------------------------------ batch backward
def _batch_backward(L, k, entry):
    """grad_features (b, c, n) of one of the two entry points, and the zero guard behind it."""
    b, c, n = k["b"], k["c"], k["n"]
    idx = dev(k["idx"])
    sizes = (b, c, n, k["m"], k["ns"])
    grad = torch.zeros(b * c * n + GUARD, device="cuda")
    if entry == "plain":                         # feature rows 3.. of (b, 3 + c, cols): batch stride (3 + c) * cols
        g = dev(k["g"])
        L.call("mgar_query_group_batch_bwd", *sizes, L.fptr(g), L.iptr(idx), L.fptr(grad), L.stream_of(g))
    else:                                        # (b, c, cols) on its own: batch stride c * cols
        g = dev(k["g"][:, 3:])
        L.call("mgar_query_group_proj_batch_bwd", *sizes, L.fptr(g), L.iptr(idx), L.fptr(grad), L.stream_of(g))
    torch.cuda.synchronize()
    assert (grad[b * c * n:] == 0).all(), "wrote behind grad_features"
    return grad[:b * c * n].view(b, c, n)


def _check_batch_backward(L, k, tag):
    n, cols = k["n"], k["cols"]
    g = k["g"][:, 3:].astype(np.float64)
    want, cnt, sabs = R.qg_scatter_batch_ref(g, k["idx"], n)
    untouched = np.broadcast_to(cnt == 0, want.shape)
    got = {e: _batch_backward(L, k, e) for e in ("plain", "proj")}
    lds = n <= QC.LDS_MAX_N
    if lds:
        bound = R.qg_fixed_point_scatter_bound(want, cnt, np.abs(g).max(axis=2, keepdims=True), cols)
        same_bits("%s LDS bwd second run" % tag, _batch_backward(L, k, "plain"), got["plain"])
        same_bits("%s LDS bwd proj entry == plain entry" % tag, got["proj"], got["plain"])
    else:
        bound = R.qg_atomic_scatter_bound(want, cnt, sabs)
    for e in got:
        within("%s %s bwd %s" % (tag, "LDS" if lds else "atomic", e), got[e], want, bound)
        assert (got[e].cpu().numpy()[untouched] == 0).all(), "a cell nobody references is not 0"
    return cnt


@pytest.mark.parametrize("cols", sorted(QC.BWD_COLS))
@pytest.mark.parametrize("n", QC.BWD_N)
def test_batch_backward_windows_threshold_and_atomic(L, n, cols):
    cnt = _check_batch_backward(L, QC.batch_bwd_case(n, cols), "n%d cols%d" % (n, cols))
    assert cnt.max() > 8 and (cnt == 0).any()


@pytest.mark.parametrize("n,cell", [(18433, 18432), (40000, 39999)], ids=["lds_lone_cell_of_window_2", "atomic"])
def test_batch_backward_every_column_on_one_cell(L, n, cell):
    cnt = _check_batch_backward(L, QC.batch_bwd_case(n, 4096, single_cell=cell), "single cell n%d" % n)
    assert cnt.max() == 4096 and (cnt > 0).sum() == QC.BWD_B


# ------------------------------------------------------------------------------------------------ stack
def _stack_chain_fp32(k):
    rows = R.stack_source_rows(k["xyz_cnt"], k["new_cnt"], k["idx"])
    live = (rows[:, 0] >= 0)[:, None, None]
    src = np.where(rows >= 0, rows, 0)
    rel = np.where(live, k["xyz"][src] - k["new_xyz"][:, None, :], np.float32(0))
    feat = np.where(live, k["feats"][src], np.float32(0))

    def channel_major(a):
        return np.ascontiguousarray(a.transpose(2, 0, 1).reshape(a.shape[2], rows.size).astype(np.float32))
    return channel_major(rel), channel_major(feat), rows


def _strided(rows_np, ld, dtype=torch.float32, fill=float("nan")):
    """(pointer tensor, whole buffer, view): the rows at row stride ld, starting STACK_BASE_OFFSET elements into a
    `fill`ed buffer with a guard behind.  The pointer tensor starts at the first row."""
    n, c = rows_np.shape
    off = QC.STACK_BASE_OFFSET
    buf = torch.full((off + n * ld + GUARD,), fill, dtype=dtype, device="cuda")
    view = buf[off:off + n * ld].view(n, ld)
    view[:, :c] = dev(rows_np).to(dtype)
    return buf[off:], buf, view


def _stack_args(L, k):
    t = {key: dev(k[key]) for key in ("xyz", "xyz_cnt", "new_xyz", "new_cnt", "idx")}
    head = (k["B"], k["M"], k["C"], k["ns"],
            L.fptr(t["xyz"]), L.iptr(t["xyz_cnt"]), L.fptr(t["new_xyz"]), L.iptr(t["new_cnt"]))
    return t, head


def _stack_refs(k, wx):
    return R.query_group_stack_ref(k["xyz"], k["xyz_cnt"], k["new_xyz"], k["new_cnt"], k["feats"], k["idx"], wx)


@pytest.mark.parametrize("C", QC.STACK_C)
@pytest.mark.parametrize("layout", sorted(QC.STACK_NEW_CNT))
def test_stack_forward_plain_proj_and_bf16(L, layout, C):
    k = QC.stack_case(layout, C)
    T, ld = k["M"] * k["ns"], C + QC.STACK_LD_PAD
    t, head = _stack_args(L, k)
    st = L.stream_of(t["xyz"])
    idx = L.iptr(t["idx"])
    rel32, feat32, _ = _stack_chain_fp32(k)
    feats, wx = dev(k["feats"]), dev(k["wx"]) if C else nans(1)
    # plain (ld = C by definition of the entry point)
    out = nans((3 + C) * T)
    L.call("mgar_query_group_stack_fwd", *head, L.fptr(feats) if C else None, idx, L.fptr(out), st)
    # proj: zf rows at stride C + 5 from a base 3 floats into the buffer; the padding is NaN, so reading it shows
    zf, _, _ = _strided(k["feats"], ld)
    rel_out, y_out, y_only = nans(3 * T), nans(C * T), nans(C * T)
    L.call("mgar_query_group_proj_stack_fwd", *head, L.fptr(zf), ld, L.fptr(wx), idx, L.fptr(rel_out), L.fptr(y_out), st)
    L.call("mgar_query_group_proj_stack_fwd", *head, L.fptr(zf), ld, L.fptr(wx), idx, None, L.fptr(y_only), st)
    # bf16 twins, and the fp32 kernels on the bf16-rounded payload
    fb = dev(feats.bfloat16().cpu().view(torch.int16).numpy()).view(BF16)
    fb32 = dev(fb.float().cpu().numpy())
    out32, outb = nans((3 + C) * T), nans((3 + C) * T, BF16)
    L.call("mgar_query_group_stack_fwd", *head, L.fptr(fb32) if C else None, idx, L.fptr(out32), st)
    L.call("mgar_query_group_stack_fwd_bf16", *head, L.pptr(fb, BF16) if C else None, idx, L.pptr(outb, BF16), st)
    if C:
        rounded = fb32.cpu().numpy()
        zf32, _, _ = _strided(rounded, ld)
        zfb, _, _ = _strided(rounded, ld, BF16)
        rel_b, y_b, y32 = nans(3 * T, BF16), nans(C * T, BF16), nans(C * T)
        L.call("mgar_query_group_proj_stack_fwd", *head, L.fptr(zf32), ld, L.fptr(wx), idx, None, L.fptr(y32), st)
        L.call("mgar_query_group_proj_stack_fwd_bf16", *head, L.pptr(zfb, BF16), ld, L.fptr(wx), idx,
               L.pptr(rel_b, BF16), L.pptr(y_b, BF16), st)
    guards_intact()
    same_bits("plain stack fwd", out.view(3 + C, T), dev(np.concatenate([rel32, feat32], 0)))
    rel64, y64 = _stack_refs(k, k["wx"])
    bound = R.qg_proj_fwd_bound(torch.from_numpy(feat32), k["wx"], rel64)
    same_bits("proj stack fwd rel", rel_out.view(3, T), dev(rel32))
    if C:
        within("proj stack fwd y", y_out.view(C, T), y64, bound)
        same_bits("proj stack fwd y without rel_out", y_only, y_out)
        assert (y_out.view(C, T)[:, dev(np.repeat(k["empty"], k["ns"]))] == 0).all()
    else:
        assert torch.isnan(y_out).all() and torch.isnan(y_only).all()
    same_bits("plain stack fwd bf16", outb, out32.bfloat16())
    if C:
        same_bits("proj stack fwd bf16 y", y_b, y32.bfloat16())
        same_bits("proj stack fwd bf16 rel", rel_b, rel_out.bfloat16())


@pytest.mark.parametrize("C", QC.STACK_C)
@pytest.mark.parametrize("layout", sorted(QC.STACK_NEW_CNT))
def test_stack_backward_plain_and_proj(L, layout, C):
    k = QC.stack_case(layout, C)
    N, ld, off = k["N"], C + QC.STACK_LD_PAD, QC.STACK_BASE_OFFSET
    t, _ = _stack_args(L, k)
    st = L.stream_of(t["xyz"])
    rows = R.stack_source_rows(k["xyz_cnt"], k["new_cnt"], k["idx"])
    want, cnt, sabs = R.qg_scatter_stack_ref(k["g"][3:], rows, N)
    bound = R.qg_atomic_scatter_bound(want, cnt, sabs)
    sizes = (k["B"], k["M"], C, k["ns"])
    counts = (L.iptr(t["idx"]), L.iptr(t["new_cnt"]), L.iptr(t["xyz_cnt"]))
    # plain: the feature rows 3.. of (3 + C, M * ns) into (N, C)
    g = dev(k["g"])
    grad = torch.zeros(N * C + GUARD, device="cuda")
    L.call("mgar_query_group_stack_bwd", *sizes, L.fptr(g), *counts, L.fptr(grad), st)
    # proj: (C, M * ns) into rows of stride C + 5 from an unaligned base
    gy = dev(k["g"][3:]) if C else nans(1)
    zp, zbuf, zview = _strided(np.zeros((N, C), np.float32), ld, fill=0.0)
    L.call("mgar_query_group_proj_stack_bwd", *sizes, L.fptr(gy), *counts, L.fptr(zp), ld, st)
    torch.cuda.synchronize()
    assert (grad[N * C:] == 0).all() and (zview[:, C:] == 0).all()
    assert (zbuf[:off] == 0).all() and (zbuf[off + N * ld:] == 0).all()
    if not C:
        return
    assert cnt.max() > 8 and (cnt == 0).any()
    for what, got in (("plain", grad[:N * C].view(N, C)), ("proj", zview[:, :C])):
        within("stack bwd %s" % what, got, want, bound)
        assert (got.cpu().numpy()[cnt[:, 0] == 0] == 0).all(), "a row nobody references is not 0"


# ------------------------------------------------------------------------------------------------ tile statistics
@pytest.mark.parametrize("C", [c for c in QC.STACK_C if c])
@pytest.mark.parametrize("variant", ["centred_with_empty_tile", "shift100_scale0.1"])
def test_stack_forward_stats_partials_and_finalised_statistics(L, variant, C):
    shifted = variant != "centred_with_empty_tile"
    k = QC.stack_case("tiles", C, 100.0, 0.1, dense=True) if shifted else QC.stack_case("tiles", C)
    T, ld, eps = k["M"] * k["ns"], C + QC.STACK_LD_PAD, 1e-5
    nt = T // 128
    t, head = _stack_args(L, k)
    st = L.stream_of(t["xyz"])
    idx = L.iptr(t["idx"])
    wx = dev(k["wx"])
    zf, _, _ = _strided(k["feats"], ld)
    rel_out, y_out, y_plain, stats = nans(3 * T), nans(C * T), nans(C * T), nans(C * nt * 2)
    L.call("mgar_query_group_proj_stack_fwd_stats", *head, L.fptr(zf), ld, L.fptr(wx), idx,
           L.fptr(rel_out), L.fptr(y_out), L.fptr(stats), st)
    L.call("mgar_query_group_proj_stack_fwd", *head, L.fptr(zf), ld, L.fptr(wx), idx, None, L.fptr(y_plain), st)
    guards_intact()
    same_bits("fwd_stats y == fwd y", y_out, y_plain)
    _, y64 = _stack_refs(k, k["wx"])
    rel64, gathered = _stack_refs(k, None)
    within("fwd_stats y", y_out.view(C, T), y64, R.qg_proj_fwd_bound(gathered, k["wx"], rel64))
    y = y_out.view(C, T).double().cpu()                       # the statistics are those of the tensor the kernel wrote
    tile_mean, tile_m2, mean, var = R.qg_tile_stats_ref(y)
    dmean, dm2 = R.qg_tile_stats_bounds(y)
    part = stats.view(C, nt, 2)
    within("tile mean", part[:, :, 0], tile_mean, dmean)
    within("tile M2", part[:, :, 1], tile_m2, dm2)
    if not shifted:
        assert (part[:, QC.STACK_EMPTY_TILE] == 0).all()      # the all-empty tile: mean and M2 exactly 0
    else:
        assert (mean.abs() > 50.0 * var.sqrt()).all()
    mean_d, invstd_d = nans(C), nans(C)
    nws = L.raw("mgar_bn_stats_from_partials_workspace_floats", nt, C)
    ws = nans(nws) if nws else None
    L.call("mgar_bn_stats_from_partials", L.fptr(stats), nt, C, T, 128, eps, 0.1, L.fptr(ws) if nws else None,
           L.fptr(mean_d), L.fptr(invstd_d), None, None, None, st)
    guards_intact()
    bmean, binv = R.qg_final_stats_bounds(y, eps)
    within("finalised mean", mean_d, mean, bmean)
    within("finalised invstd", invstd_d, (var + eps) ** -0.5, binv)


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_raise_and_launch_nothing(L):
    """Every rejected call is an accepted call with exactly one argument replaced; the accepted calls run first."""
    C = 7
    k, ragged = QC.stack_case("tiles", C), QC.stack_case("ragged", C)
    T = k["M"] * k["ns"]
    t, head = _stack_args(L, k)
    st = L.stream_of(t["xyz"])
    idx, counts = L.iptr(t["idx"]), (L.iptr(t["idx"]), L.iptr(t["new_cnt"]), L.iptr(t["xyz_cnt"]))
    zf, wx, gy = dev(k["feats"]), dev(k["wx"]), dev(k["g"][3:])
    zfb = dev(zf.bfloat16().cpu().view(torch.int16).numpy()).view(BF16)
    rel_out, y_out, stats, yb = nans(3 * T), nans(C * T), nans(C * (T // 128) * 2), nans(C * T, BF16)
    grad = torch.zeros(k["N"] * C, device="cuda")
    # batch entries: b = 3 accepted, b = 65 536 not; the buffers are sized for the large b all the same
    big = 65536
    hx, hq, hf = (torch.zeros(big * s, device="cuda") for s in (3, 3, 1))
    hfb = torch.zeros(big, dtype=BF16, device="cuda")
    hi = torch.zeros(big, dtype=torch.int32, device="cuda")
    one = dev(np.ones((1, 3), np.float32))
    ho, hy, hob, hyb = nans(big * 4), nans(big), nans(big * 4, BF16), nans(big, BF16)
    hg = torch.zeros(big, device="cuda")
    ones = (1, 1, 1, 1)                                       # c, n, npoints, nsample
    geo = (L.fptr(hx), L.fptr(hq))
    f32, bf = (L.fptr(zf), C, L.fptr(wx), idx), (L.pptr(zfb, BF16), C, L.fptr(wx), idx)
    good = {
        "mgar_query_group_proj_stack_fwd": (*head, *f32, L.fptr(rel_out), L.fptr(y_out), st),
        "mgar_query_group_proj_stack_fwd_bf16": (*head, *bf, None, L.pptr(yb, BF16), st),
        "mgar_query_group_proj_stack_fwd_stats": (*head, *f32, L.fptr(rel_out), L.fptr(y_out), L.fptr(stats), st),
        "mgar_query_group_proj_stack_bwd": (k["B"], k["M"], C, k["ns"], L.fptr(gy), *counts, L.fptr(grad), C, st),
        "mgar_query_group_batch_fwd": (3, *ones, *geo, L.fptr(hf), L.iptr(hi), L.fptr(ho), st),
        "mgar_query_group_batch_fwd_bf16": (3, *ones, *geo, L.pptr(hfb, BF16), L.iptr(hi), L.pptr(hob, BF16), st),
        "mgar_query_group_proj_batch_fwd": (3, *ones, *geo, L.fptr(hf), L.fptr(one), L.iptr(hi), None, L.fptr(hy), st),
        "mgar_query_group_proj_batch_fwd_bf16": (3, *ones, *geo, L.pptr(hfb, BF16), L.fptr(one), L.iptr(hi), None,
                                                 L.pptr(hyb, BF16), st),
        "mgar_query_group_batch_bwd": (3, *ones, L.fptr(ho), L.iptr(hi), L.fptr(hg), st),
        "mgar_query_group_proj_batch_bwd": (3, *ones, L.fptr(hy), L.iptr(hi), L.fptr(hg), st),
    }
    ZF_LD, WX_STACK, WX_BATCH, BWD_LD, M_ARG = 9, 10, 8, 9, 1     # positions in the argument lists
    bad = [  # (entry point, position, replacement, what the message must say)
        ("mgar_query_group_proj_stack_fwd_stats", M_ARG, ragged["M"], r"M \* nsample % 128"),
        ("mgar_query_group_proj_stack_fwd", ZF_LD, C - 1, "zf_ld < C"),
        ("mgar_query_group_proj_stack_fwd_bf16", ZF_LD, C - 1, "zf_ld < C"),
        ("mgar_query_group_proj_stack_fwd_stats", ZF_LD, C - 1, "zf_ld < C"),
        ("mgar_query_group_proj_stack_bwd", BWD_LD, C - 1, "ld < C"),
        ("mgar_query_group_proj_stack_fwd", WX_STACK, None, "null pointer"),
        ("mgar_query_group_proj_stack_fwd_bf16", WX_STACK, None, "null pointer"),
        ("mgar_query_group_proj_stack_fwd_stats", WX_STACK, None, "null pointer"),
        ("mgar_query_group_proj_batch_fwd", WX_BATCH, None, "null pointer"),
        ("mgar_query_group_proj_batch_fwd_bf16", WX_BATCH, None, "null pointer"),
    ] + [(name, 0, big, "> 65535") for name in good if "_batch_" in name]
    assert {name for name, _, _, _ in bad} == set(good)
    for name, args in good.items():                           # the accepted calls are accepted
        L.call(name, *args)
    torch.cuda.synchronize()
    outputs = (rel_out, y_out, stats, yb, ho, hy, hob, hyb)
    for o in outputs:
        as_int, bits = NAN_BITS[o.dtype]
        o.view(as_int).fill_(bits)
    grad.zero_()
    hg.zero_()
    was_on = L._KT_STATE["on"]
    L.kernel_timers(enable=True)
    L.kernel_timers()                                         # reading resets the counters
    try:
        for name, pos, value, message in bad:
            args = list(good[name])
            assert args[pos] != value
            args[pos] = value
            with pytest.raises(L.MgarError, match=message):
                L.call(name, *args)
        torch.cuda.synchronize()
        launched = L.kernel_timers()
    finally:
        L.kernel_timers(enable=was_on)
    assert launched == {}, "a rejected call launched a kernel"
    guards_intact()
    for o in outputs:
        assert torch.isnan(o).all()
    assert (grad == 0).all() and (hg == 0).all()
