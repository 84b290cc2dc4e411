"""Per-scene multi-head attention (csrc/scene_mha.hip), what can be checked without a GPU: the two entry points are declared,
exported and documented, the ABI version did not move, their argument checks return codes before any device call, the
float64 reference the GPU tests compare against is nn.MultiheadAttention's own arithmetic, the op layer refuses what the
kernel cannot mirror, and the committed reference fixture passes its generator's assertions."""
import os
import re

import numpy as np
import pytest
import torch

import scene_mha_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mgar_scene_mha_fwd", "mgar_scene_mha_bwd")


def test_header_declares_both_symbols_and_the_abi_is_still_22():
    from multimodal_gar_amd import _lib
    text = open(os.path.join(ROOT, "include", "mgar_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 22 and _lib._fns["mgar_abi_version"]() == 22
    assert len(_lib._fns["mgar_scene_mha_fwd"].argtypes) == 15 and len(_lib._fns["mgar_scene_mha_bwd"].argtypes) == 19


def test_integration_document_names_both_symbols():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert "`%s`" % name in text, name


def test_argument_checks_return_codes_before_any_device_call():
    from multimodal_gar_amd import _lib
    fwd, bwd = _lib._fns["mgar_scene_mha_fwd"], _lib._fns["mgar_scene_mha_bwd"]
    N = None

    def both(S, rows, H, hd, pairs, ld):
        return (fwd(S, rows, H, hd, N, N, pairs, N, N, N, ld, 0.125, N, N, N),
                bwd(S, rows, H, hd, N, N, pairs, N, N, N, ld, 0.125, N, N, N, N, N, N, N))
    assert both(1, 4, 8, 32, 16, 512) == (-3, -3)          # head_dim != 64
    assert both(1, 4, 8, 64, 16, 130) == (-3, -3)          # ld % 4 != 0
    assert both(1, 4, 8, 64, 16, 256) == (-3, -3)          # the heads do not fit the row
    assert both(-1, 4, 8, 64, 16, 512) == (-1, -1)
    assert both(1, 4, 0, 64, 16, 512) == (-1, -1)
    assert both(0, 0, 8, 64, 0, 512) == (0, 0)             # empty: OK, nothing launched
    assert both(3, 0, 8, 64, 0, 512) == (0, 0)
    assert both(1, 4, 8, 64, 16, 512) == (-1, -1)          # null pointers


@pytest.mark.parametrize("counts,H", [((1, 5, 0, 9), 2), ((7,), 8), ((3, 2), 1)])
def test_reference_is_multihead_attention_in_float64(counts, H):
    """Identity in- and out-projections: the module's output IS the attention core, so this pins the head split (head h =
    columns [64 h, 64 h + 64)) and the scaling (1 / sqrt(64)) of mha_reference."""
    E = H * MC.HEAD_DIM
    q, k, v, _ = MC.inputs(list(counts), H, seed=3)
    mha = torch.nn.MultiheadAttention(E, H).double().eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
        mha.out_proj.bias.zero_()
    out, att = MC.mha_reference(q, k, v, counts, H, 1.0 / MC.HEAD_DIM ** 0.5)
    assert out.shape == (sum(counts), E) and att.shape == (H, sum(n * n for n in counts))
    r0 = m0 = 0
    for n in counts:
        if n:
            rows = slice(r0, r0 + n)
            with torch.no_grad():
                want, w = mha(q[rows].double(), k[rows].double(), v[rows].double(), need_weights=True,
                              average_attn_weights=False)
            assert (out[rows] - want).abs().max() <= 1e-12
            assert (att[:, m0:m0 + n * n].reshape(H, n, n) - w).abs().max() <= 1e-12
        r0 += n
        m0 += n * n


def test_op_layer_refuses_what_the_kernel_cannot_mirror():
    from multimodal_gar_amd.scene_mha_ops import _check_module
    MHA = torch.nn.MultiheadAttention
    _check_module(MHA(512, 8))
    _check_module(MHA(512, 8, dropout=0.1).eval())          # dropout is inactive in eval mode
    for bad in (MHA(512, 4), MHA(512, 16), MHA(512, 8, dropout=0.1), MHA(512, 8, add_bias_kv=True),
                MHA(512, 8, add_zero_attn=True), MHA(512, 8, kdim=256, vdim=256)):
        with pytest.raises(NotImplementedError):
            _check_module(bad)


def test_workload_takes_a_modality():
    from multimodal_gar_amd import workload as W
    cfg = W.model_cfg(5, 1024, modality="LiDAR").GAR_MODEL
    assert (cfg.MODALITY, cfg.FEAT_NORM, cfg.FEATURE_DIM, cfg.HIDDEN_DIM) == ("LiDAR", False, 512, 512)
    cfg = W.model_cfg(5, 1024).GAR_MODEL
    assert (cfg.MODALITY, cfg.FEAT_NORM, cfg.FEATURE_DIM) == ("Multi", True, 1024)
    with pytest.raises(ValueError):
        W.model_cfg(5, 1024, modality="Radar")
    model = W.ClipModel(5, 1024, modality="LiDAR")
    assert not hasattr(model.net, "RGB_backbone") and hasattr(model.net, "LiDAR_backbone")


def test_committed_fixture_passes_the_generators_assertions():
    G = np.load(MC.GOLDEN)
    gap = MC.check_fixture(G)
    print("smallest |A_theta - 0.5| over the valid off-diagonal entries: %.4f" % gap)
    assert len(G.files) == 4 * 2 * 2 * 16 + 2 * 2 * 4 + 3
    assert os.path.getsize(MC.GOLDEN) < 1 << 20
