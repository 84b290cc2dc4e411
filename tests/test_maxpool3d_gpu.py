"""3-D max pooling (csrc/maxpool3d.hip and the channels-last kernel of csrc/channels_last.hpp): mgar_maxpool3d_same_fwd,
mgar_maxpool3d_valid_fwd, mgar_maxpool3d_same_fwd_cl and their bf16 twins against torch_refs.maxpool3d_ref -- the reference's
"same" padding rule, then the maximum of every window in float64 -- on the cases of channels_last_cases.py.  A maximum is
exact: results must be EQUAL as values (bf16 in, bf16 out loses nothing either), and a NaN in a window is its maximum, as in
torch.max_pool3d.  tests/test_channels_last_cpu.py shows that the reference is F.pad -> max_pool3d and that every case takes
the kernel it names.

Every output starts as payload NaNs -- so an output the kernel never wrote fails the comparison -- with a guard behind it that
must keep its bits (nans(), guards_intact() of tests/test_query_group_gpu.py).

Which case covers which edge:
  stride-1 quad kernel  W = 4 (one quad: left and right edge at once), W = 8; H = 1; T in 1..4 around the three-slice register
                        window; kt in {1, 2, 3} x st in {1, 2}
  stride-2 quad kernel  W = 8 (one quad), 16; T odd / even (front padding 1 / 0 in t); kh in {1, 3}
  one thread per output Wo % 4 != 0 (W = 6, 12 at stride 2), kt = 4, k = s = 2, NC = 65 536 (the gate of the quad kernels)
  all-negative input    "valid" differs from "same" wherever the window leaves the input
  grid-stride loops     more outputs than the capped grids hold at once (bf16, generated on the device, against
                        torch.nn.functional.max_pool3d of the padded device tensor)
  channels-last         C in {4, 8, 24} x (T, H, W) in {(1,1,1), (2,3,5), (3,4,4)} x the three I3D geometries and (2,2,2)/(2,2,2)
  non-finite            a NaN in the interior, at corners where the window also holds padding, in the element a quad loads as
                        its left / right neighbour, and in slice t - 2 of a kt = 3 window: exactly the windows that hold it
                        are NaN.  With fmaxf throughout, none is."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import channels_last_cases as CC
import torch_refs as R
from test_bn_act_gpu import F32, _release, devt, twin  # noqa: F401
from test_query_group_gpu import BF16, L, _fresh_guards, dev, guards_intact, nans  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL = -1
NCDHW = ("mgar_maxpool3d_same_fwd", "mgar_maxpool3d_valid_fwd")
CL = "mgar_maxpool3d_same_fwd_cl"
PAD_OF = {"mgar_maxpool3d_same_fwd": 0.0, "mgar_maxpool3d_valid_fwd": -np.inf, CL: 0.0}


def out_dims(dims, s):
    return tuple(-(-n // st) for n, st in zip(dims, s))


def pool(L, entry, x, NC, thw, k, s):
    """x (NC, T, H, W) device tensor, fp32 or bf16 -> y (NC, To, Ho, Wo)."""
    od = out_dims(thw, s)
    y = nans(NC * od[0] * od[1] * od[2], x.dtype)
    L.call(twin(entry, x.dtype), L.pptr(x, x.dtype), NC, *thw, *k, *s, L.pptr(y, x.dtype), L.stream_of(x))
    guards_intact()
    return y.view((NC,) + od)


def pool_cl(L, x, N, thw, C, k, s):
    """x (N, T, H, W, C) -> y (N, To, Ho, Wo, C)."""
    od = out_dims(thw, s)
    y = nans(N * od[0] * od[1] * od[2] * C, x.dtype)
    L.call(twin(CL, x.dtype), L.pptr(x, x.dtype), N, *thw, C, *k, *s, L.pptr(y, x.dtype), L.stream_of(x))
    guards_intact()
    return y.view((N,) + od + (C,))


def equal_values(what, got, want):
    """got (device tensor) equals want (float64 numpy) as values, NaN where and only where want is NaN."""
    got = got.float().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: %d outputs NaN, %d expected, %d differ" % (what, nan_g.sum(), nan_w.sum(), (nan_g != nan_w).sum())
    bad = (got != want) & ~nan_w
    assert not bad.any(), "%s: %d of %d outputs differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def check_ncdhw(L, x, NC, thw, k, s, tag):
    """All four NCDHW entries on x (numpy fp32); bf16: the same values after rounding x to bf16."""
    xb = dev(x).bfloat16()
    for dtype, xd, xv in ((F32, dev(x), x), (BF16, devt(xb), xb.float().cpu().numpy())):
        for entry in NCDHW:
            equal_values("%s %s %s" % (tag, entry, dtype), pool(L, entry, xd, NC, thw, k, s), R.maxpool3d_ref(xv, k, s, PAD_OF[entry]))


# ------------------------------------------------------------------------------------------------ NCDHW
@pytest.mark.parametrize("name", sorted(CC.POOL_CASES))
def test_maxpool3d_same_and_valid(L, name):
    c = CC.pool_case(name)
    thw = (c["T"], c["H"], c["W"])
    assert CC.pool_route(c["NC"], *thw, c["k"], c["s"]) == c["route"]
    check_ncdhw(L, c["x"], c["NC"], thw, c["k"], c["s"], name)
    if c["negative"]:
        same, valid = (pool(L, e, dev(c["x"]), c["NC"], thw, c["k"], c["s"]) for e in NCDHW)
        assert (valid < 0).all() and (same == 0).any() and ((same == 0) | (same == valid)).all()


def test_maxpool3d_grid_stride_loop_of_the_scalar_kernel(L):
    """2 x 2 x 2049 x 2049 = 16 793 604 outputs > 65 536 blocks x 256 threads: the loop takes a second turn.  bf16, 34 MB in,
    34 MB out; kernel (2, 2, 2) at stride 1 pads one element behind every axis."""
    NC, thw, k, s = 2, (2, 2049, 2049), (2, 2, 2), (1, 1, 1)
    assert NC * thw[0] * thw[1] * thw[2] > 65536 * 256 and CC.pool_route(NC, *thw, k, s) == "scalar"
    torch.manual_seed(3)
    x = (torch.randn((NC,) + thw, device="cuda") - 0.5).bfloat16()
    pads = [R.same_pads(n, kk, ss) for n, kk, ss in zip(thw, k, s)]
    for entry in NCDHW:
        want = F.max_pool3d(F.pad(x[None].float(), pads[2] + pads[1] + pads[0], value=PAD_OF[entry]), k, s)[0].bfloat16()
        got = pool(L, entry, x, NC, thw, k, s)
        assert torch.equal(got, want), "%s: %d outputs differ" % (entry, int((got != want).sum()))
        del want, got


# ------------------------------------------------------------------------------------------------ channels-last
@pytest.mark.parametrize("thw", CC.POOL_CL_THW, ids=lambda t: "%dx%dx%d" % t)
@pytest.mark.parametrize("C", CC.POOL_CL_C)
def test_maxpool3d_same_channels_last(L, C, thw):
    for k, s in CC.POOL_CL_GEOMETRIES:
        c = CC.pool_cl_case(C, thw, k, s)
        tag = "cl C%d %s k%s s%s" % (C, thw, k, s)
        xb = dev(c["x_cl"]).bfloat16()
        for dtype, xd, xv in ((F32, dev(c["x_cl"]), c["x"]), (BF16, devt(xb), np.moveaxis(xb.float().cpu().numpy(), -1, 1))):
            want = np.moveaxis(R.maxpool3d_ref(xv, k, s, 0.0), 1, -1)
            equal_values("%s %s" % (tag, dtype), pool_cl(L, xd, c["N"], thw, C, k, s), want)


def test_maxpool3d_channels_last_grid_stride_loop(L):
    """2 x 1025 x 2049 positions x 8 channels = 8 400 900 float4 groups > 32 768 blocks x 256 threads.  bf16, 67 MB in."""
    N, thw, C, k, s = 1, (2, 1025, 2049), 8, (2, 2, 2), (1, 1, 1)
    assert N * thw[0] * thw[1] * thw[2] * (C // 4) > 32768 * 256
    torch.manual_seed(4)
    x = (torch.randn((N,) + thw + (C,), device="cuda") - 0.5).bfloat16()
    pads = [R.same_pads(n, kk, ss) for n, kk, ss in zip(thw, k, s)]
    want = F.max_pool3d(F.pad(x.permute(0, 4, 1, 2, 3).float(), pads[2] + pads[1] + pads[0]), k, s).permute(0, 2, 3, 4, 1).bfloat16()
    got = pool_cl(L, x, N, thw, C, k, s)
    assert torch.equal(got, want.contiguous()), "%d outputs differ" % int((got != want).sum())


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_leave_the_output_untouched(L):
    x, y = dev(np.zeros((1, 2, 2, 2, 8), np.float32)), nans(64)
    p, q, st = x.data_ptr(), y.data_ptr(), L.stream_of(x)
    for sfx in ("", "_bf16"):
        for bad in ((0, 3, 3, 1, 1, 1), (3, 0, 3, 1, 1, 1), (3, 3, 0, 1, 1, 1), (3, 3, 3, 0, 1, 1), (3, 3, 3, 1, 0, 1), (3, 3, 3, 1, 1, 0)):
            assert L.raw("mgar_maxpool3d_same_fwd" + sfx, p, 8, 2, 2, 2, *bad, q, st) == EINVAL
            assert L.raw("mgar_maxpool3d_valid_fwd" + sfx, p, 8, 2, 2, 2, *bad, q, st) == EINVAL
            assert L.raw("mgar_maxpool3d_same_fwd_cl" + sfx, p, 1, 2, 2, 2, 8, *bad, q, st) == EINVAL
        assert L.raw("mgar_maxpool3d_same_fwd_cl" + sfx, p, 1, 2, 2, 4, 6, 3, 3, 3, 1, 1, 1, q, st) == EINVAL      # C % 4 != 0
        assert L.raw("mgar_maxpool3d_same_fwd_cl" + sfx, None, 0, 2, 2, 2, 8, 3, 3, 3, 1, 1, 1, None, st) == 0
        assert L.raw("mgar_maxpool3d_same_fwd" + sfx, None, 0, 2, 2, 2, 3, 3, 3, 1, 1, 1, None, st) == 0
    guards_intact()
    assert torch.isnan(y).all()


# ------------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("site", range(len(CC.POOL_NAN_SITES)), ids=lambda i: "%s@%d.%d.%d" % ((CC.POOL_NAN_SITES[i][0],) + CC.POOL_NAN_SITES[i][1]))
def test_a_nan_is_the_maximum_of_exactly_the_windows_that_hold_it(L, site):
    """In plane 1 of 3; planes 0 and 2 stay finite.  All four NCDHW entries, fp32 and bf16; then the same tensor read as
    channels-last with four copies of every plane as channels (C = 12)."""
    name, (t, h, w), what = CC.POOL_NAN_SITES[site]
    c = CC.pool_case(name)
    thw = (c["T"], c["H"], c["W"])
    x = c["x"].copy()
    x[1, t, h, w] = np.nan
    want = R.maxpool3d_ref(x, c["k"], c["s"], 0.0)
    assert np.isnan(want[1]).any() and not np.isnan(want[[0, 2]]).any()
    check_ncdhw(L, x, c["NC"], thw, c["k"], c["s"], "%s NaN at %s (%s)" % (name, (t, h, w), what))
    x5 = np.repeat(x[None], 4, axis=1)                                # (1, 12, T, H, W)
    x_cl = np.ascontiguousarray(np.moveaxis(x5, 1, -1))
    for dtype in (F32, BF16):
        xd = devt(dev(x_cl).to(dtype))
        xv = np.moveaxis(xd.float().cpu().numpy(), -1, 1)
        equal_values("cl %s NaN at %s %s" % (name, (t, h, w), dtype), pool_cl(L, xd, 1, thw, 12, c["k"], c["s"]),
                     np.moveaxis(R.maxpool3d_ref(xv, c["k"], c["s"], 0.0), 1, -1))
