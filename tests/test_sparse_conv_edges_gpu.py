"""Op-level edge tests of csrc/sparse_conv.hip against the float64 references of tests/sparse_conv_cases.py (pinned on the CPU by
tests/test_sparse_conv_cpu.py): voxel hash, rulebook and output sites, the two gather-GEMM kernels, the pair-list builder, both
weight-gradient kernels, the pair-list forward / data-gradient kernel with more than one tile per item, the whole op, and
non-finite containment.

Index results are compared bit for bit.  Every value is compared per ELEMENT: |got - ref| <= gamma(n + m) S + 1e-30 (see the
cases module) -- a wrong value in a small-magnitude row or channel cannot hide behind the global maximum, and a row without
any product must be an exact zero.  `record_error` logs for each comparison the share of its bound that was used."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparse_conv_cases as C
from conftest import record_error

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(what, got, ref, S, n, m):
    got = host(got).astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    ratio = np.abs(got - ref) / C.bound(n, m, S)
    used = float(ratio.max()) if ratio.size else 0.0
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, "%s: err / bound %.3g at %s" % (what, used, np.unravel_index(ratio.argmax(), ratio.shape))


def gather(nbr, x, w, flip, register):
    from multimodal_gar_amd import _lib as L, sparse_ops
    K, cin, cout = w.shape
    L.call("mgar_spconv_set_register_gather", register)
    try:
        return sparse_ops._gather_gemm(nbr.shape[0], K, cin, cout, x, nbr, w, flip)
    finally:
        L.call("mgar_spconv_set_register_gather", 1)


def rulebook_from_table(nbr):
    """A Rulebook around a given table, built without __init__: what Rulebook.pairs() reads."""
    from multimodal_gar_amd import sparse_ops
    rb = sparse_ops.Rulebook.__new__(sparse_ops.Rulebook)
    rb.nbr, rb.K, rb._pairs, rb.subm, rb.inv = nbr, nbr.shape[1], None, True, None
    return rb


@functools.lru_cache(maxsize=None)
def subm_table(n):
    """nbr of the submanifold k3 rulebook over exactly n sites (reference), shared and left unchanged"""
    return C.rulebook_ref(C.rows_case(n), C.ROWS_GRID, 3, 1, 1, True)[2]


@functools.lru_cache(maxsize=None)
def geometry_ref(i):
    case, gname, coords, shape, batch, subm, kernel, stride, padding = C.geometry_cases()[i]
    return C.rulebook_ref(coords, shape, kernel, stride, padding, subm)


# ---- hash -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.hash_cases()))
def test_voxel_hash_lookup_equals_the_dict(name):
    """Load exactly 0.5 (n8, n512) and the next capacity (n9, n513), N = 0 and 1, duplicated coordinates (smallest row wins),
    out-of-grid and negative-batch rows at build time; queries present, absent, outside each face, b < 0."""
    from multimodal_gar_amd.sparse_ops import VoxelHash
    coords, q, want = C.hash_cases()[name]
    h = VoxelHash(dev(coords), C.HASH_SHAPE)
    if name in ("n8", "n512"):
        assert h.capacity == 2 * len(coords)
    assert np.array_equal(host(h.lookup(dev(q))), want)
    assert host(h.lookup(dev(q[:0]))).shape == (0,)
    assert len(coords) == 0 or (want >= 0).sum() >= min(len(coords), 30)


# ---- rulebook ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.GEOMETRY_IDS)), ids=C.GEOMETRY_IDS)
def test_rulebook_equals_the_dict_reference(i):
    """out_indices, out_shape, nbr and the inverse table, bit for bit: faces and corners, one-cell-thick grids, odd extents
    under stride 2, a dropped last plane, empty samples, adjacent keys across samples, no input / no output site, keys > 2^31."""
    from multimodal_gar_amd.sparse_ops import Rulebook
    case, gname, coords, shape, batch, subm, kernel, stride, padding = C.geometry_cases()[i]
    oidx, oshape, nbr, inv = geometry_ref(i)
    rb = Rulebook(dev(coords), shape, batch, kernel, stride, padding, subm)
    assert list(rb.out_shape) == oshape
    assert rb.out_indices.dtype == torch.int32 and np.array_equal(host(rb.out_indices).reshape(-1, 4), oidx)
    assert rb.nbr.dtype == torch.int32 and tuple(rb.nbr.shape) == nbr.shape and np.array_equal(host(rb.nbr), nbr)
    if subm:
        assert rb.inverse_table() is None           # the forward table with mirrored offsets serves (pinned on the CPU)
    else:
        got = rb.inverse_table()
        assert tuple(got.shape) == inv.shape and np.array_equal(host(got), inv)
    assert rb.pair_count() == int((nbr >= 0).sum())


# ---- gather-GEMM ------------------------------------------------------------------------------------------------------------
def gather_both_kernels(what, nbr, cin, cout, seed, unaligned=False):
    K = nbr.shape[1]
    rng = np.random.default_rng(seed)
    n_src = int(nbr.max()) + 1 if nbr.size and nbr.max() >= 0 else 1
    x, w = C.wide_range(rng, (max(n_src, nbr.shape[0]), cin)), C.weights(rng, K, cin, cout)
    nbr_d, x_d, w_d = dev(nbr), dev(x), dev(w)
    takes, float4 = C.register_kernel_takes(cin, cout)
    for flip in (0, 1):
        ref, S, n = C.gather_gemm_ref(nbr, x, w, flip)
        outs = {}
        for register in (1, 0):
            outs[register] = gather(nbr_d, x_d, w_d, flip, register)
            check("%s %dx%d flip %d register %d" % (what, cin, cout, flip, register), outs[register], ref, S, n, 2)
        if not takes:                                # outside the channel table the switch changes nothing
            assert torch.equal(outs[1], outs[0])
        if unaligned:
            # the storage starts one float past a 16-byte boundary: the float4 path must not be taken (the LDS kernel stands
            # in), the scalar path and the LDS kernel read the same values: bit-equal to the aligned run of the same kernel
            buf = torch.empty(x_d.numel() + 1, dtype=torch.float32, device="cuda")
            xu = buf[1:].view(x_d.shape)
            xu.copy_(x_d)
            assert xu.data_ptr() % 16 == 4 and xu.is_contiguous()
            for register in (1, 0):
                got = gather(nbr_d, xu, w_d, flip, register)
                same_as = outs[0] if (register == 0 or (takes and float4)) else outs[1]
                assert torch.equal(got, same_as), (cin, cout, flip, register)


@pytest.mark.parametrize("n", C.ROWS)
def test_gather_gemm_row_counts_at_the_tile_edges(n):
    """N = 1, 2 and one below / at / one above 32 (rows per wave), 64 (LDS kernel tile), 128 (register kernel tile), 512, 1 024:
    both kernels, float4 plan (16, 16) and scalar plan (33, 40), mirrored offsets."""
    nbr = subm_table(n)
    assert nbr.shape == (n, 27)
    for cin, cout in C.ROWS_PLANS:
        gather_both_kernels("rows %d" % n, nbr, cin, cout, 1000 + n)


@pytest.mark.parametrize("cin,cout", C.PLANS)
def test_gather_gemm_channel_plans(cin, cout):
    """Every instantiation of the register kernel on its float4 and its scalar path (with and without a C_out tail), the LDS
    kernel with 1 to 4 column blocks, C_in 128 with C_out <= 32 (falls out of the table), 128 -> 128 (above 64 KB of dynamic
    LDS); 193 rows (ragged last tile of either kernel), K = 27; and a feature buffer that is not 16-byte aligned."""
    gather_both_kernels("plan", subm_table(C.PLAN_ROWS), cin, cout, cin * 131 + cout, unaligned=True)


@pytest.mark.parametrize("K", C.SMALL_K)
def test_gather_gemm_small_kernel_volumes(K):
    """K = 1 (no prefetch step of the register kernel at all), 2, 3 (odd: the double-buffer loop ends on its first half), 8."""
    for cin, cout in C.PLANS_SMALL_K:
        gather_both_kernels("K %d" % K, C.small_table(K), cin, cout, 77 + K)


# ---- pair-list builder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.builder_tables()))
def test_pair_list_builder_on_synthetic_tables(name):
    """sp_pairs_{count,scan,fill} and the host cut into items: per-offset counts at the edges of the 64-pair tile and the
    4 096-pair item, offsets with no pair, 64-row groups and 512-row blocks with none, a ragged last block, one row."""
    from multimodal_gar_amd import _lib as L
    nbr = C.builder_tables()[name]
    K = nbr.shape[1]
    rb = rulebook_from_table(dev(nbr))
    pair_i, pair_o, items_dw, start_dw, n_dw, items_fw, start_fw = rb.pairs()
    want_i, want_o, counts = C.pair_lists(nbr)
    p = int(counts.sum())
    assert rb._pair_count == p
    assert np.array_equal(host(pair_i)[:p], want_i) and np.array_equal(host(pair_o)[:p], want_o)
    offs = np.concatenate([[0], np.cumsum(counts)])
    chunk = L.raw("mgar_spconv_pair_chunk")
    assert chunk == 4096
    for items, start, n_items, c in ((host(items_dw), host(start_dw), n_dw, chunk), (host(items_fw), list(start_fw), None, 64)):
        start = [int(s) for s in start]
        assert len(start) == K + 1 and start[0] == 0 and (n_items is None or n_items == start[-1])
        for k in range(K):
            its = items[start[k]:start[k + 1]]
            assert len(its) == -(-int(counts[k]) // c)
            at = offs[k]
            for kk, b, e, _ in its.tolist():                 # contiguous cover of the offset's pairs, full items but the last
                assert kk == k and b == at and e == min(at + c, offs[k + 1]) and e > b
                at = e
            assert at == offs[k + 1]


# ---- weight gradient --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_table_on_device():
    nbr, counts, _ = C.main_table()
    rb = rulebook_from_table(dev(nbr))
    rb.pairs()
    return nbr, counts, rb


def dw_inputs(cin, cout):
    rng = np.random.default_rng(cin * 257 + cout)
    return C.wide_range(rng, (C.MAIN_ROWS, cin)), C.wide_range(rng, (C.MAIN_ROWS, cout))


def pairs_dw(rb, x_d, g_d):
    from multimodal_gar_amd import _lib as L
    pair_i, pair_o, items, item_start, n_items = rb.pairs()[:5]
    K, cin, cout = rb.K, x_d.shape[1], g_d.shape[1]
    part = torch.empty((max(n_items, 1), cin, cout), dtype=torch.float32, device="cuda")
    dw = torch.full((K, cin, cout), 7.0, dtype=torch.float32, device="cuda")          # fully written: no 7 survives
    L.call("mgar_spconv_pairs_dw", n_items, K, cin, cout, L.fptr(x_d), L.fptr(g_d), L.iptr(pair_i), L.iptr(pair_o), L.iptr(items),
           L.iptr(item_start), L.fptr(part), L.fptr(dw), L.stream_of(x_d))
    return dw


def table_dw(nbr_d, x_d, g_d):
    from multimodal_gar_amd import _lib as L
    n, K = nbr_d.shape
    cin, cout = x_d.shape[1], g_d.shape[1]
    nchunk = L.raw("mgar_spconv_dw_chunks", n)
    part = torch.full((max(nchunk, 1), K, cin, cout), 7.0, dtype=torch.float32, device="cuda")
    L.call("mgar_spconv_dw", n, K, cin, cout, L.fptr(x_d), L.iptr(nbr_d), L.fptr(g_d), L.fptr(part), L.stream_of(x_d))
    return part.sum(0), nchunk


@pytest.mark.parametrize("cin,cout", C.DW_PAIR_PLANS)
def test_pair_list_weight_gradient_on_the_main_table(cin, cout):
    """spconv_pairs_dw_kernel<4, 8, 16, 32> + the reduction: items of 1, 63 .. 65, 127 .. 129, 191 .. 193 pairs (1 to 4 tiles: the
    three-slot index ring wraps), 4 095 .. 4 097 (a second item of one pair) and 8 200 (three partials); 128 x 128 above 64 KB."""
    nbr, counts, rb = main_table_on_device()
    x, g = dw_inputs(cin, cout)
    x_d, g_d = dev(x), dev(g)
    ref, S, n = C.dw_ref(nbr, x, g)
    partials = -(-np.array(counts) // 4096)
    got = pairs_dw(rb, x_d, g_d)
    check("pairs dw %dx%d" % (cin, cout), got, ref, S, n, (partials + 2).reshape(-1, 1, 1))
    assert torch.equal(got, pairs_dw(rb, x_d, g_d))
    assert 0 in counts and (host(got)[np.array(counts) == 0] == 0).all()


@pytest.mark.parametrize("cin,cout", C.DW_TABLE_PLANS)
def test_table_weight_gradient_on_the_main_table(cin, cout):
    """spconv_dw_kernel: 8 200 rows = one full 8 192-row chunk + 8 rows, 64-row tiles without a pair skipped, channel counts
    with tails in both dimensions, padded 128 x 128 above 64 KB."""
    nbr, counts, rb = main_table_on_device()
    x, g = dw_inputs(cin, cout)
    x_d, g_d = dev(x), dev(g)
    ref, S, n = C.dw_ref(nbr, x, g)
    got, nchunk = table_dw(rb.nbr, x_d, g_d)
    assert nchunk == 2
    check("table dw %dx%d" % (cin, cout), got, ref, S, n, nchunk + 2)
    assert torch.equal(got, table_dw(rb.nbr, x_d, g_d)[0])
    assert (host(got)[np.array(counts) == 0] == 0).all()


# ---- pair-list forward / data gradient, items of more than one tile ------------------------------------------------------------
def pairs_gemm(src, pair_src, pair_dst, items, starts, w, n_dst):
    from multimodal_gar_amd import _lib as L
    K, cs, cd = w.shape
    dst = torch.zeros((n_dst, cd), dtype=torch.float32, device="cuda")
    start_host = (ctypes.c_int * len(starts))(*starts)
    L.call("mgar_spconv_pairs_gemm", K, cs, cd, L.fptr(src), L.iptr(pair_src), L.iptr(pair_dst), L.iptr(items),
           ctypes.cast(start_host, ctypes.c_void_p), L.fptr(w), L.fptr(dst), L.stream_of(src))
    return dst


@pytest.mark.parametrize("transpose", [False, True], ids=["forward", "dgrad"])
@pytest.mark.parametrize("cin,cout", C.PAIR_GEMM_PLANS)
def test_pair_list_gemm_with_hand_made_items(cin, cout, transpose):
    """spconv_pairs_gemm_kernel with ONE item of 1 .. 4 096 pairs per offset (ntiles 1, 1, 2, 2, 3, 3, 4, 64: prefetch and index
    ring; Rulebook.pairs() only ever cuts 64-pair items here) and a second offset that updates some of the same rows."""
    from multimodal_gar_amd import _lib as L
    for p in C.PAIR_ITEM_SIZES:
        p1 = min(p, 65)
        n_out, n_in = p + 9, p + 7
        nbr = C.pair_item_table(p)
        pair_i, pair_o, counts = C.pair_lists(nbr)
        items = dev(np.array([[0, 0, p, 0], [1, p, p + p1, 0]], np.int32))
        rng = np.random.default_rng(p + cin)
        x, g, w = C.wide_range(rng, (n_in, cin)), C.wide_range(rng, (n_out, cout)), C.weights(rng, 2, cin, cout)
        if not transpose:
            args = (dev(x), dev(pair_i), dev(pair_o), items, [0, 1, 2], dev(w), n_out)
            ref, S, n = C.gather_gemm_ref(nbr, x, w)
            untouched = (nbr < 0).all(1)
        else:
            args = (dev(g), dev(pair_o), dev(pair_i), items, [0, 1, 2], dev(np.ascontiguousarray(w.transpose(0, 2, 1))), n_in)
            ref, S, n = C.dgrad_ref(nbr, g, w, n_in)
            untouched = ~np.isin(np.arange(n_in), nbr[nbr >= 0])
            if cout & (cout - 1):                    # documented precondition: C_src a power of two
                with pytest.raises(L.MgarError, match="power of two"):
                    pairs_gemm(*args)
                continue
        got = pairs_gemm(*args)
        check("pairs gemm %s %dx%d item %d" % ("dgrad" if transpose else "fwd", cin, cout, p), got, ref, S, n, 2)
        assert untouched.sum() == (7 if transpose else 9) and (host(got)[untouched] == 0).all()      # rows outside every pair keep the caller's zeros
        assert torch.equal(got, pairs_gemm(*args))


# ---- whole op ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.GEOMETRY_IDS)), ids=C.GEOMETRY_IDS)
def test_sparse_conv3d_forward_backward_on_the_geometry_cases(i, monkeypatch):
    """sparse_ops.sparse_conv3d, output + both gradients, over pair lists and over tables, power-of-two and other channel
    counts; no input site and no output site give correctly shaped empty outputs and all-zero gradients."""
    from multimodal_gar_amd import sparse_ops
    case, gname, coords, shape, batch, subm, kernel, stride, padding = C.geometry_cases()[i]
    oidx, oshape, nbr, inv = geometry_ref(i)
    kk = C.triple(kernel)
    K, n_in, n_out = nbr.shape[1], len(coords), len(oidx)
    coords_d = dev(coords)
    for cin, cout in C.CONV_CHANNELS:
        x, w = C.conv_tensors(case, gname, n_in, K, cin, cout)
        cot = C.conv_cotangent(n_out, cout)
        refs = (C.gather_gemm_ref(nbr, x, w), C.dgrad_ref(nbr, cot, w, n_in), C.dw_ref(nbr, x, cot))
        w_param = np.ascontiguousarray(w.reshape(*kk, cin, cout).transpose(4, 0, 1, 2, 3))          # (Cout, kz, ky, kx, Cin)
        for pairs in (True, False):
            monkeypatch.setattr(sparse_ops, "PAIRS_FORWARD", pairs)
            monkeypatch.setattr(sparse_ops, "PAIRS_DGRAD", pairs)
            f, ww = dev(x).requires_grad_(True), dev(w_param).requires_grad_(True)
            out, gidx, gshape = sparse_ops.sparse_conv3d(f, coords_d, list(shape), batch, ww, kernel, stride, padding, subm, {}, "k")
            assert list(gshape) == oshape and np.array_equal(host(gidx).reshape(-1, 4), oidx)
            assert tuple(out.shape) == (n_out, cout) and out.dtype == torch.float32
            (out * dev(cot)).sum().backward()
            assert f.grad is not None and tuple(f.grad.shape) == (n_in, cin) and tuple(ww.grad.shape) == w_param.shape
            what = "%s %s %dx%d pairs %d" % (case, gname, cin, cout, pairs)
            check(what + " out", out, *refs[0], 2)
            check(what + " d features", f.grad, *refs[1], 2)
            check(what + " d weight", ww.grad.permute(1, 2, 3, 4, 0).reshape(K, cin, cout), *refs[2], 1 + 2)
            if n_in == 0 or n_out == 0:
                assert not host(f.grad).any() and not host(ww.grad).any()


# ---- non-finite containment -------------------------------------------------------------------------------------------------
def bits(t):
    return host(t).view(np.int32)


@pytest.mark.parametrize("cin,cout", [(16, 16), (33, 40), (5, 128)])
def test_nan_in_one_input_row_reaches_exactly_its_readers_forward(cin, cout):
    """A NaN in one channel of one input row: exactly the output rows whose table names that row are NaN, in every channel;
    every other row -- in the same 64- / 128-row MFMA tile included -- is bit-equal to the clean run.  Both kernels."""
    nbr = subm_table(C.PLAN_ROWS)
    rng = np.random.default_rng(cin + 3 * cout)
    x, w = C.wide_range(rng, (C.PLAN_ROWS, cin)), C.weights(rng, 27, cin, cout)
    nbr_d, w_d = dev(nbr), dev(w)
    for r0, c0 in ((70, cin - 1), (5, 0)):
        readers = (nbr == r0).any(1)
        tile = np.arange(C.PLAN_ROWS) // 64 == r0 // 64
        assert readers[r0] and 2 <= readers.sum() < 40 and (tile & ~readers).sum() > 20
        bad = x.copy()
        bad[r0, c0] = np.nan
        for register in (1, 0):
            clean, got = gather(nbr_d, dev(x), w_d, 0, register), gather(nbr_d, dev(bad), w_d, 0, register)
            assert np.isnan(host(got)[readers]).all() and not np.isnan(host(got)[~readers]).any()
            assert np.array_equal(bits(got)[~readers], bits(clean)[~readers])


@pytest.mark.parametrize("kernel,cin,cout", [("pairs", 16, 16), ("pairs", 128, 128), ("table", 24, 40), ("table", 128, 128)])
def test_nan_in_one_input_row_reaches_exactly_its_offsets_weight_gradient(kernel, cin, cout):
    """The same NaN in the weight gradient: exactly the entries (k, c0, :) of the offsets k that pair that row are NaN."""
    nbr = subm_table(C.PLAN_ROWS)
    rng = np.random.default_rng(cin + 5 * cout)
    x, g = C.wide_range(rng, (C.PLAN_ROWS, cin)), C.wide_range(rng, (C.PLAN_ROWS, cout))
    rb = rulebook_from_table(dev(nbr))
    run = (lambda a: pairs_dw(rb, dev(a), dev(g))) if kernel == "pairs" else (lambda a: table_dw(rb.nbr, dev(a), dev(g))[0])
    r0, c0 = 70, cin - 3
    want = np.zeros((27, cin, cout), bool)
    want[(nbr == r0).any(0), c0, :] = True
    assert 2 <= (nbr == r0).any(0).sum() < 27
    bad = x.copy()
    bad[r0, c0] = np.nan
    clean, got = run(x), run(bad)
    assert np.array_equal(np.isnan(host(got)), want) and not np.isnan(host(clean)).any()
    assert np.array_equal(bits(got)[~want], bits(clean)[~want])
