"""CPU tests of the boundary: libmgar_hip.so loads without a GPU and exports every symbol that
include/mgar_ops.h declares (no compute calls here), argument validation returns error codes
instead of exiting, and the host-side index plumbing is correct."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mgar_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    syms = declared_symbols()
    assert len(syms) >= 25
    for must in ["mgar_ball_query_batch", "mgar_ball_query_stack", "mgar_fps_batch", "mgar_fps_stack",
                 "mgar_voxel_query_stack", "mgar_three_nn_batch", "mgar_group_points_grad_stack",
                 "mgar_roi_align_fwd", "mgar_dafm_attn_bwd", "mgar_gatv2_fwd"]:
        assert must in syms


def test_library_exports_every_declared_symbol():
    from multimodal_gar_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(cdll, name), "libmgar_hip.so does not export %s" % name
    assert sorted(_lib.exported_symbols()) == declared_symbols()
    assert cdll.mgar_abi_version() == _lib.ABI_VERSION


def test_binding_return_types_match_the_header():
    """ctypes' restype per entry point is the header's declared return type (a suffix rule gave
    mgar_pointwise_dw_bnbwd_workspace_floats -- an `int` -- a 64-bit restype)."""
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = dict((name, ret) for ret, name in
                re.findall(r"^\s*(long long|int|const char \*)\s*(mgar_[a-z0-9_]+)\s*\(", text, flags=re.M))
    assert len(decl) > 100
    want = {"long long": ctypes.c_longlong, "int": ctypes.c_int, "const char *": ctypes.c_char_p}
    for name, fn in _lib._fns.items():
        assert fn.restype is want[decl[name]], name
    assert {n for n, f in _lib._fns.items() if f.restype is ctypes.c_longlong} == {n for n, r in decl.items() if r == "long long"}


def test_binding_argument_types_match_the_header():
    """argtypes per entry point against expectations written out by hand from include/mgar_ops.h: every scalar type of the
    ABI and its awkward shapes.  An int where the header says long long (strides, totals) or a float for a double
    truncates silently; nothing else would notice before wrong numbers on a GPU."""
    from multimodal_gar_amd import _lib
    I, F, D, LL, P, S = (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p,
                         ctypes.c_char_p)
    interp_into = (I, [I, I, I, I, P, P, P, P, LL, P])
    expect = {
        "mgar_ktimer_add_flops": (I, [I, D]),
        "mgar_ktimer_read": (I, [I, P, P, P, P, I]),
        "mgar_ktimer_name": (S, [I]),
        "mgar_last_error": (S, []),
        "mgar_abi_version": (I, []),
        "mgar_spconv_pair_chunk": (I, []),
        "mgar_point_grid_workspace_bytes": (LL, [I, LL]),
        "mgar_rowmajor_dw_workspace_floats": (I, [LL, I, I]),
        "mgar_ball_query_batch": (I, [I, I, I, F, I, P, P, P, P]),
        # host arrays radii / nsamples, then new_xyz, xyz, `int *const *idx`, stream
        "mgar_ball_query_multi_batch": (I, [I, I, I, I, P, P, P, P, P, P]),
        # dpool, three long long strides, then pointers and sizes
        "mgar_bn_act_maxpool_bwd_strided": (I, [P, LL, LL, LL, P, P, P, P, I, I, I, I, P, P, P, I, P, P, P, P, P]),
        "mgar_three_interpolate_batch_into": interp_into,
        "mgar_three_interpolate_batch_into_bf16": interp_into,
        "mgar_image_resize_normalize_u8": (I, [I, I, I, I, I, P, P, P, P, P, P, P, LL, LL, I, P]),
    }
    for name, (restype, argtypes) in expect.items():
        fn = _lib._fns[name]
        assert fn.restype is restype, name
        assert len(fn.argtypes) == len(argtypes) and all(a is b for a, b in zip(fn.argtypes, argtypes)), name


def test_bf16_twins_share_their_base_signature():
    from multimodal_gar_amd import _lib
    assert len(_lib.BF16_TWINS) == 27
    assert _lib.BF16_TWINS == {n[:-5] for n in _lib._fns if n.endswith("_bf16")}
    for base in _lib.BF16_TWINS:
        twin = _lib._fns[base + "_bf16"]
        assert list(twin.argtypes) == list(_lib._fns[base].argtypes), base
        assert twin.restype is _lib._fns[base].restype, base


def test_header_parser_is_strict():
    """A type the binding does not know must fail the import, not bind as something plausible."""
    from multimodal_gar_amd import _lib
    version = "#define MGAR_ABI_VERSION 7\n"
    I, F, D, LL, P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p
    ok = version + """
        /* a comment naming mgar_not_a_function(int) */
        #define MGAR_SOMETHING 3
        extern "C" {
        int mgar_a(void);   // trailing mgar_comment(unsigned n);
        long long mgar_b(int n, long long total,
                         float r, double d,
                         const float *x, int *const *idx, const unsigned char *arg, void *stream);
        const char *mgar_c(int id);
        }
    """
    assert _lib._parse_header(ok) == (7, {"mgar_a": (I, []), "mgar_b": (LL, [I, LL, F, D, P, P, P, P]),
                                          "mgar_c": (ctypes.c_char_p, [I])})
    for bad in ("int mgar_x(unsigned n);", "int mgar_x(size_t n);", "int mgar_x(struct mgar_box box);",
                "int mgar_x(mgar_box box);", "int mgar_x(int (*callback)(int));", "unsigned mgar_x(int n);",
                "char *mgar_x(int n);", "float *mgar_x(int n);", "int mgar_x(int);", "int mgar_x(int n); int mgar_x(int n);",
                "struct mgar_box { int n; };"):
        with pytest.raises(ImportError):
            _lib._parse_header(version + bad)
    with pytest.raises(ImportError):
        _lib._parse_header("int mgar_x(int n);")        # no MGAR_ABI_VERSION


def test_invalid_arguments_return_codes_not_exit():
    """The reference exit(-1)s on bad input (ball_query.cpp:14-26); the C ABI returns a code.
    Argument checks run before any HIP call, so this is safe without a GPU."""
    from multimodal_gar_amd import _lib
    assert _lib._fns["mgar_ball_query_batch"](1, 10, 10, 1.0, 0, None, None, None, None) == -3   # nsample < 1
    assert _lib._fns["mgar_ball_query_batch"](-1, 10, 10, 1.0, 4, None, None, None, None) == -1
    assert _lib._fns["mgar_fps_batch"](2, 0, 5, None, None, None, None) == -1                    # m > 0 from empty
    assert _lib._fns["mgar_three_nn_batch"](0, 0, 0, None, None, None, None, None) == 0          # empty is a no-op
    assert _lib._fns["mgar_gatv2_fwd"](4, 8, 100, None, None, None, None, None, 0.2, None, None, None, None) in (-1, -3)
    with pytest.raises(_lib.MgarError):
        _lib.call("mgar_group_points_batch", -1, 1, 1, 1, 1, None, None, None, None)
    assert b"negative" in _lib._cdll.mgar_last_error()


def test_ops_refuse_cpu_tensors():
    from multimodal_gar_amd import _lib
    from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb
    with pytest.raises(_lib.MgarError):
        pb.ball_query(1.0, 4, torch.zeros(1, 8, 3), torch.zeros(1, 2, 3))


def test_edges_to_csr_matches_reference_graph_construction():
    from multimodal_gar_amd.graph_ops import edges_to_csr
    n = 5
    comb = torch.combinations(torch.arange(n), r=2)
    ei = torch.cat((comb, torch.flip(comb, [1])), 0).T        # model/gat_model.py:1085-1092
    rowptr, col = edges_to_csr(ei, n)
    assert rowptr.tolist() == [0, 5, 10, 15, 20, 25]
    for i in range(n):
        assert sorted(col[rowptr[i]:rowptr[i + 1]].tolist()) == list(range(n))  # all sources + self loop


def test_scene_offsets_and_roi_format():
    from multimodal_gar_amd.dafm_ops import scene_offsets
    from multimodal_gar_amd.vision_ops import convert_boxes_to_roi_format
    so, do = scene_offsets([3, 1, 4], "cpu")
    assert so.tolist() == [0, 3, 4, 8] and do.tolist() == [0, 9, 10]
    rois = convert_boxes_to_roi_format([torch.ones(2, 4), torch.zeros(1, 4)])
    assert rois.shape == (3, 5) and rois[:, 0].tolist() == [0.0, 0.0, 1.0]
