"""The C ABI of csrc/conv3d_bf16.hip (3x3x3 / stride-1 / "same" convolution of bf16 NCDHW payloads on the bf16 MFMA) without a
GPU: the two entry points are declared and exported, they are not `_bf16` twins of the fp32 kernel (other signature, called
by name), the workspace size is the documented one, and unsupported shapes return MGAR_EINVAL before any device call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgar_conv3d_k3_bf16_workspace_bytes", "mgar_conv3d_k3_bf16_fwd")
MGAR_OK, MGAR_EINVAL = 0, -1


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
    assert ws.restype is LL and list(ws.argtypes) == [I, I]
    assert fwd.restype is I and list(fwd.argtypes) == [P, I, I, I, I, I, P, I, P, P, P]
    assert _lib.ABI_VERSION >= 14


def test_entry_points_are_not_bf16_twins():
    from multimodal_gar_amd import _lib
    assert len(_lib.BF16_TWINS) == 27
    for name in NAMES:
        assert not name.endswith("_bf16")
        assert name not in _lib.BF16_TWINS and name[:-5] not in _lib.BF16_TWINS
    assert "mgar_conv3d_k3_fwd" not in _lib.BF16_TWINS


def test_workspace_bytes():
    """28 672 bytes per (64 output channels, 8 input channels): 14 k-steps x 2 channel blocks x 2 half-waves x 32 rows x 8 bf16."""
    from multimodal_gar_amd import _lib
    ws = _lib._fns[NAMES[0]]
    for cin, cout in ((0, 64), (64, 0), (-8, 64), (64, -1), (0, 0)):
        assert ws(cin, cout) == 0
    block = 14 * 2 * 2 * 32 * 8 * 2
    assert block == 28672
    assert ws(8, 64) == block
    assert ws(8, 1) == block                       # a partial channel group is a whole block
    assert ws(64, 192) == 3 * 8 * block
    assert ws(24, 64) == 3 * block
    assert ws(96, 208) == 4 * 12 * block
    assert ws(160, 320) == 5 * 20 * block


def test_unsupported_shapes_return_einval_without_a_device():
    from multimodal_gar_amd import _lib
    fwd = _lib._fns[NAMES[1]]
    one = ctypes.c_void_p(16)                      # non-null, never dereferenced: every check below fails before a device call
    assert fwd(one, 1, 12, 2, 4, 6, one, 8, one, one, None) == MGAR_EINVAL       # C_in % 8 != 0
    assert b"multiple of 8" in _lib._cdll.mgar_last_error()
    assert fwd(one, 1, 4, 2, 4, 6, one, 8, one, one, None) == MGAR_EINVAL
    assert fwd(one, 1, 8, 2, 4, 7, one, 8, one, one, None) == MGAR_EINVAL        # odd W
    assert fwd(one, 1, 8, 0, 4, 6, one, 8, one, one, None) == MGAR_EINVAL        # empty volume
    assert fwd(one, -1, 8, 2, 4, 6, one, 8, one, one, None) == MGAR_EINVAL
    assert fwd(one, 1, 8, 2, 4, 6, one, 0, one, one, None) == MGAR_EINVAL
    for k in range(4):                                                           # a null pointer with N > 0
        ptrs = [one, one, one, one]
        ptrs[k] = None
        assert fwd(ptrs[0], 1, 8, 2, 4, 6, ptrs[1], 8, ptrs[2], ptrs[3], None) == MGAR_EINVAL
        assert b"null pointer" in _lib._cdll.mgar_last_error()


def test_empty_batch_is_a_no_op():
    from multimodal_gar_amd import _lib
    fwd = _lib._fns[NAMES[1]]
    assert fwd(None, 0, 8, 2, 4, 6, None, 8, None, None, None) == MGAR_OK
    assert fwd(None, 0, 12, 2, 4, 6, None, 8, None, None, None) == MGAR_EINVAL   # the shape rules hold for an empty batch too


def test_timer_row_and_source_map():
    from multimodal_gar_amd import _lib, op_timer
    names = [_lib.raw("mgar_ktimer_name", i).decode() for i in range(_lib.raw("mgar_ktimer_count"))]
    assert "conv3d_bf16_kernel" in names and len(set(names)) == len(names)
    src = [v for v in vars(op_timer).values() if isinstance(v, dict) and "conv3d_wino_kernel" in v]
    assert src and src[0].get("conv3d_bf16_kernel") == "conv3d_bf16.hip"
