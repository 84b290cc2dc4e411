"""The C ABI and the host routing of csrc/sparse_conv_bf16.hip (forward gather-GEMM of the sparse convolution for bf16 rows on
the bf16 MFMA) without a GPU: the two entry points are declared, exported and bound, they are not `_bf16` twins, the workspace
size is the documented one, unsupported plans and bad arguments are refused before any device call, the timer row exists, the
bound of the device test is satisfiable by a correct implementation, and fp32 / gradient-carrying features never reach the
new entry point."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import sparse_conv_bf16_cases as B
import sparse_conv_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgar_spconv_bf16_workspace_bytes", "mgar_spconv_bf16_fwd")
MGAR_OK, MGAR_EINVAL, MGAR_EUNSUPPORTED = 0, -1, -3
BAD_PLANS = [(27, cin, 32) for cin in (4, 24, 144)] + [(27, 32, cout) for cout in (0, 129)] + [(K, 32, 32) for K in (0, 344)]


def test_header_declares_and_library_exports_both_symbols():
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
        assert name in _lib.exported_symbols()
    I, LL, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    ws, fwd = _lib._fns[NAMES[0]], _lib._fns[NAMES[1]]
    assert ws.restype is LL and list(ws.argtypes) == [I, I, I]
    assert fwd.restype is I and list(fwd.argtypes) == [I, I, I, I, P, P, P, I, P, P, P]
    assert _lib.ABI_VERSION >= 17


def test_entry_points_are_not_bf16_twins():
    from multimodal_gar_amd import _lib
    assert len(_lib.BF16_TWINS) == 27
    for name in NAMES:
        assert not name.endswith("_bf16")
        assert name not in _lib.BF16_TWINS and name[:-5] not in _lib.BF16_TWINS
    assert "mgar_spconv_gather_gemm" not in _lib.BF16_TWINS


def test_workspace_bytes():
    """K * (C_in / 16) * ceil(C_out / 32) * 1 024: per offset, 16-channel k-step and 32-column block, 64 lanes x 16 bytes."""
    from multimodal_gar_amd import _lib
    ws = _lib._fns[NAMES[0]]
    assert ws(1, 16, 1) == 1024
    assert ws(27, 16, 16) == 27 * 1024
    assert ws(27, 64, 64) == 27 * 4 * 2 * 1024
    assert ws(27, 64, 128) == 27 * 4 * 4 * 1024
    assert ws(27, 128, 128) == 27 * 8 * 4 * 1024
    assert ws(27, 48, 40) == 27 * 3 * 2 * 1024
    assert ws(27, 112, 33) == 27 * 7 * 2 * 1024
    assert ws(343, 128, 128) == 343 * 32 * 1024
    for K in (1, 3, 27, 343):
        for cin in range(16, 129, 16):
            for cout in (1, 31, 32, 33, 64, 65, 96, 97, 128):
                assert ws(K, cin, cout) == K * (cin // 16) * -(-cout // 32) * 1024
    for K, cin, cout in BAD_PLANS + [(27, -16, 32), (27, 32, -1), (-1, 32, 32), (27, 0, 32), (27, 8, 32), (27, 136, 32)]:
        assert ws(K, cin, cout) == 0, (K, cin, cout)


def test_unsupported_plans_and_bad_arguments_are_refused_without_a_device():
    from multimodal_gar_amd import _lib
    fwd = _lib._fns[NAMES[1]]
    one = ctypes.c_void_p(16)                      # non-null, 16-byte aligned, never dereferenced: every call below fails first
    for K, cin, cout in BAD_PLANS:
        for No in (5, 0):                          # the plan rules hold for an empty launch too
            assert fwd(No, K, cin, cout, one, one, one, 0, one, one, None) in (MGAR_EUNSUPPORTED, MGAR_EINVAL), (No, K, cin, cout)
    for cin in (4, 24, 144):
        assert fwd(5, 27, cin, 32, one, one, one, 0, one, one, None) == MGAR_EUNSUPPORTED
    assert fwd(5, 27, 32, 129, one, one, one, 0, one, one, None) == MGAR_EUNSUPPORTED
    assert fwd(-1, 27, 32, 32, one, one, one, 0, one, one, None) == MGAR_EINVAL
    assert fwd(5, 0, 32, 32, one, one, one, 0, one, one, None) == MGAR_EINVAL
    assert fwd(5, 27, 32, 0, one, one, one, 0, one, one, None) == MGAR_EINVAL
    for k in range(5):                             # each null pointer with No > 0
        ptrs = [one] * 5
        ptrs[k] = None
        assert fwd(5, 27, 32, 32, ptrs[0], ptrs[1], ptrs[2], 0, ptrs[3], ptrs[4], None) == MGAR_EINVAL
        assert b"null pointer" in _lib._cdll.mgar_last_error()
    for addr in (2, 8, 18):                        # a misaligned `in`
        assert fwd(5, 27, 32, 32, ctypes.c_void_p(addr), one, one, 0, one, one, None) == MGAR_EINVAL
        assert b"aligned" in _lib._cdll.mgar_last_error()


def test_empty_launch_is_a_no_op():
    from multimodal_gar_amd import _lib
    fwd = _lib._fns[NAMES[1]]
    assert fwd(0, 27, 32, 32, None, None, None, 0, None, None, None) == MGAR_OK
    assert fwd(0, 27, 64, 128, None, None, None, 1, None, None, None) == MGAR_OK


def test_timer_row_and_source_map():
    from multimodal_gar_amd import _lib, op_timer
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "spconv_bf16_kernel" in names and "spconv_gemm" in names and len(set(names)) == len(names)
    assert op_timer.KERNEL_SOURCES.get("spconv_bf16_kernel") == "sparse_conv_bf16.hip"
    assert os.path.exists(os.path.join(ROOT, "multimodal_gar_amd", "csrc", "sparse_conv_bf16.hip"))


@pytest.mark.parametrize("name", sorted(B.value_cases()))
def test_bound_is_satisfiable_by_a_correct_implementation(name):
    """fp32 accumulation of the exact products, offsets ascending and descending, one bf16 rounding: inside the bound on every
    value case of the device test; rows without a product are exact zeros."""
    nbr, x, w, flip = B.operands(name)
    assert np.array_equal(B.to_bf16(x), x) and np.array_equal(B.to_bf16(w), w)
    ref, S, n = C.gather_gemm_ref(nbr, x, w, flip)
    lim = B.bound(ref, S, n)
    for descending in (False, True):
        got = B.emulate(nbr, x, w, flip, descending).astype(np.float64)
        used = float((np.abs(got - ref) / lim).max())
        assert used <= 1.0, (name, descending, used)
        assert (got[n[:, 0] == 0] == 0).all()
    if name.startswith("alternate_tiles"):
        assert (n[(np.arange(len(n)) // 64) % 2 == 1] == 0).all()          # the property the case is there for


def _fake_rulebook(indices, n_out, K):
    nbr = torch.full((n_out, K), -1, dtype=torch.int32)
    return types.SimpleNamespace(in_indices=indices, kernel=(3, 3, 3), stride=(1, 1, 1), padding=(1, 1, 1), subm=True, in_shape=[4, 4, 4],
                                 K=K, nbr=nbr, out_indices=indices, out_shape=[4, 4, 4], inv=None)


def test_host_routing_on_cpu_tensors(monkeypatch):
    """fp32 features and bf16 features that need a gradient never reach mgar_spconv_bf16_fwd; bf16 features without one do, unless
    the switch is off or the plan is unsupported.  No device: L.call only records the entry point's name."""
    from multimodal_gar_amd import _lib as L, sparse_ops
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append(name) or 0)
    monkeypatch.setattr(L, "dev_ptr", lambda t, dtype=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(L, "stream_of", lambda t: None)
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    indices = torch.zeros((6, 4), dtype=torch.int32)

    def run(dtype, grad_feats=False, grad_w=False, cin=32, cout=64, no_grad=False):
        del calls[:]
        feats = torch.ones((6, cin), dtype=dtype, requires_grad=grad_feats)
        weight = torch.ones((cout, 3, 3, 3, cin), requires_grad=grad_w)
        cache = {"k": _fake_rulebook(indices, 6, 27)}
        with (torch.no_grad() if no_grad else torch.enable_grad()):
            out = sparse_ops.sparse_conv3d(feats, indices, [4, 4, 4], 1, weight, 3, 1, 1, True, cache, "k")[0]
        return out.dtype, list(calls)

    assert run(torch.float32) == (torch.float32, ["mgar_spconv_gather_gemm"])
    assert run(torch.float32, no_grad=True) == (torch.float32, ["mgar_spconv_gather_gemm"])
    assert run(torch.float32, grad_w=True) == (torch.float32, ["mgar_spconv_gather_gemm"])
    assert run(torch.bfloat16, grad_feats=True) == (torch.float32, ["mgar_spconv_gather_gemm"])
    assert run(torch.bfloat16, grad_w=True) == (torch.float32, ["mgar_spconv_gather_gemm"])
    assert run(torch.bfloat16) == (torch.bfloat16, ["mgar_spconv_bf16_fwd"])
    assert run(torch.bfloat16, grad_w=True, no_grad=True) == (torch.bfloat16, ["mgar_spconv_bf16_fwd"])
    assert run(torch.bfloat16, cin=24, cout=40) == (torch.float32, ["mgar_spconv_gather_gemm"])          # unsupported plan
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", False)
    assert run(torch.bfloat16) == (torch.float32, ["mgar_spconv_gather_gemm"])
