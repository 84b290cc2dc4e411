"""The eval-mode BatchNorm [+ ReLU] store of the sparse convolution on the device: mgar_spconv_gather_gemm_affine (both fp32
kernels) and mgar_spconv_bf16_fwd_affine against the float64 reference and per-element bounds of
tests/sparse_conv_affine_cases.py (pinned as satisfiable by tests/test_sparse_conv_affine_cpu.py), bit-level properties (identity
epilogue == the plain entry point, repeatability, position independence, NaN), the SparseSequential routing around them, and
the Voxel R-CNN trunk in eval mode: fused against the unfused torch batch norm (MGAR_SPCONV_FOLD_BN off = the behaviour before
the fold), fp32 and under bf16 autocast.  `record_error` logs the share of the bound each comparison used."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import sparse_conv_affine_cases as A
import sparse_conv_bf16_cases as B
import sparse_conv_cases as C
from conftest import record_error

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PARITY = 1e-4                                   # the project's parity tolerance, max-norm relative to the reference's maximum


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared cases are read-only


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def plain_fp32(nbr_d, x_d, w_d, flip=0):
    from multimodal_gar_amd import _lib as L
    K, cin, cout = w_d.shape
    out = torch.full((nbr_d.shape[0], cout), float("nan"), dtype=torch.float32, device="cuda")
    L.call("mgar_spconv_gather_gemm", nbr_d.shape[0], K, cin, cout, L.fptr(x_d), L.iptr(nbr_d), L.fptr(w_d), int(flip), L.fptr(out),
           L.stream_of(x_d))
    return out


def affine_fp32(nbr_d, x_d, w_d, flip, scale_d, shift_d, relu):
    """mgar_spconv_gather_gemm_affine called by name; out pre-filled with NaN ("fully written")"""
    from multimodal_gar_amd import _lib as L
    K, cin, cout = w_d.shape
    out = torch.full((nbr_d.shape[0], cout), float("nan"), dtype=torch.float32, device="cuda")
    L.call("mgar_spconv_gather_gemm_affine", nbr_d.shape[0], K, cin, cout, L.fptr(x_d), L.iptr(nbr_d), L.fptr(w_d), int(flip),
           L.fptr(scale_d), L.fptr(shift_d), int(relu), L.fptr(out), L.stream_of(x_d))
    return out


def affine_bf16(nbr_d, x_bf, w_d, flip, scale_d, shift_d, relu):
    """mgar_spconv_bf16_fwd_affine called by name: x_bf (Ni, Cin) bf16, w_d fp32 -> (No, Cout) bf16"""
    from multimodal_gar_amd import _lib as L
    K, cin, cout = w_d.shape
    nbytes = L.raw("mgar_spconv_bf16_workspace_bytes", K, cin, cout)
    assert nbytes > 0
    packed = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    out = torch.full((nbr_d.shape[0], cout), float("nan"), dtype=BF, device="cuda")
    L.call("mgar_spconv_bf16_fwd_affine", nbr_d.shape[0], K, cin, cout, L.pptr(x_bf, BF), L.iptr(nbr_d), L.fptr(w_d), int(flip),
           L.fptr(scale_d), L.fptr(shift_d), int(relu), L.dev_ptr(packed, torch.uint8), L.pptr(out, BF), L.stream_of(x_bf))
    return out


def check(what, got, z, S, n, scale, shift, relu, bf16):
    got = host(got).astype(np.float64)
    ref = A.reference(z, scale, shift, relu)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    ratio = np.abs(got - ref) / A.bound(z, S, n, scale, shift, relu, bf16)
    used = float(ratio.max()) if ratio.size else 0.0
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, "%s: err / bound %.3g at %s" % (what, used, np.unravel_index(ratio.argmax(), ratio.shape))
    if relu:
        assert (got >= 0).all() and not np.signbit(got).any(), "%s: a negative pre-activation must give +0" % what


def operands(name, bf16):
    c = A.case(name, bf16)
    x_d = dev(c["x"]).to(BF) if bf16 else dev(c["x"])
    return c, dev(c["nbr"]), x_d, dev(c["w"]), dev(c["scale"]), dev(c["shift"])


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.value_cases(False)))
def test_fp32_kernel_against_float64(name):
    """The value cases of the bf16 kernel's test (channel plans at 193 rows, row counts 1 .. 1 025 around the 32 / 128 tile edges,
    K = 1, 2, 3, 8, mirrored offsets, alternate empty tiles, the 8 200-row table) plus every fp32 channel plan (register float4,
    register scalar, LDS, big LDS); scale of mixed sign with zero channels, about half of the pre-activations negative."""
    c, nbr_d, x_d, w_d, sc_d, sh_d = operands(name, False)
    for relu in (1, 0):
        got = affine_fp32(nbr_d, x_d, w_d, c["flip"], sc_d, sh_d, relu)
        check("%s relu=%d" % (name, relu), got, c["z"], c["S"], c["n"], c["scale"], c["shift"], relu, False)


@pytest.mark.parametrize("name", sorted(A.value_cases(True)))
def test_bf16_kernel_against_float64_on_the_rounded_operands(name):
    c, nbr_d, x_d, w_d, sc_d, sh_d = operands(name, True)
    assert np.array_equal(host(x_d), c["x"])
    for relu in (1, 0):
        got = affine_bf16(nbr_d, x_d, w_d, c["flip"], sc_d, sh_d, relu)
        assert got.dtype == BF
        check("%s bf16 relu=%d" % (name, relu), got, c["z"], c["S"], c["n"], c["scale"], c["shift"], relu, True)
        assert torch.equal(bits(got), bits(affine_bf16(nbr_d, x_d, w_d, c["flip"], sc_d, sh_d, relu)))      # repeatable


CONSISTENCY = sorted(A.fp32_plan_cases()) + ["rows_1_16x16", "rows_129_16x16", "rows_1025_64x128", "small_k1_48x40", "small_k8_16x16",
                                             "flip_32x64", "alternate_tiles_32x32"]


@pytest.mark.parametrize("name", CONSISTENCY)
def test_fp32_identity_epilogue_is_the_plain_entry_point_bit_for_bit(name):
    """scale = 1, shift = 0, relu = 0: the bits of mgar_spconv_gather_gemm, on the register-gather kernel (where the plan takes it)
    and on the LDS-staged kernel."""
    from multimodal_gar_amd import _lib as L
    c, nbr_d, x_d, w_d, _, _ = operands(name, False)
    cout = w_d.shape[2]
    one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
    try:
        for register_gather in (1, 0):
            L.call("mgar_spconv_set_register_gather", register_gather)
            want = plain_fp32(nbr_d, x_d, w_d, c["flip"])
            got = affine_fp32(nbr_d, x_d, w_d, c["flip"], one, zero, 0)
            assert not torch.isnan(want).any()
            assert torch.equal(bits(got), bits(want)), (name, register_gather)
            # and the epilogue is the same function of the accumulator on both kernels
            sc_d, sh_d = dev(c["scale"]), dev(c["shift"])
            full = affine_fp32(nbr_d, x_d, w_d, c["flip"], sc_d, sh_d, 1)
            v = torch.addcmul(sh_d.double(), want.double(), sc_d.double()).float()        # fmaf through float64
            assert torch.equal(bits(full), bits(torch.where(v > 0, v, torch.zeros_like(v)))), (name, register_gather)
    finally:
        L.call("mgar_spconv_set_register_gather", 1)


@pytest.mark.parametrize("cin,cout", B.ROWS_PLANS)
def test_bf16_a_rows_bits_do_not_depend_on_its_position_or_on_the_launch_size(cin, cout):
    """Row o of the 1 025-row launch == the same table row at another position (a permuted table) == the same row in a table
    extended by rows behind it == launched alone, bit for bit."""
    c, nbr_d, x_d, w_d, sc_d, sh_d = operands("rows_1025_%dx%d" % (cin, cout), True)
    nbr = c["nbr"]
    full = bits(affine_bf16(nbr_d, x_d, w_d, 0, sc_d, sh_d, 1))
    perm = np.random.default_rng(11).permutation(nbr.shape[0])
    moved = bits(affine_bf16(dev(nbr[perm]), x_d, w_d, 0, sc_d, sh_d, 1))
    assert torch.equal(moved, full[torch.from_numpy(perm).cuda()])
    for rows in (1, 31, 33, 128, 129, 640):
        head = bits(affine_bf16(dev(nbr[:rows]), x_d, w_d, 0, sc_d, sh_d, 1))
        assert torch.equal(head, full[:rows]), rows                                       # the table extended by rows after it
    for o in (0, 31, 32, 127, 128, 1024):
        alone = bits(affine_bf16(dev(nbr[o:o + 1]), x_d, w_d, 0, sc_d, sh_d, 1))
        assert torch.equal(alone[0], full[o]), o


@pytest.mark.parametrize("bf16,register_gather", [(False, 1), (False, 0), (True, 1)], ids=["fp32-register", "fp32-lds", "bf16"])
def test_nan_appears_in_exactly_the_outputs_that_name_it(bf16, register_gather):
    """One NaN element in one input row: every output row with that row in its table is NaN in every channel (zero scale
    included), no other element is; with and without ReLU.  The finite outputs behind a ReLU are >= 0 with a + sign."""
    from multimodal_gar_amd import _lib as L
    c, nbr_d, x_d, w_d, sc_d, sh_d = operands("rows_129_16x16", bf16)
    nbr = c["nbr"]
    j = int(nbr[nbr >= 0][7])
    x_d = x_d.clone()
    x_d[j, 3] = float("nan")
    named = torch.from_numpy((nbr == j).any(1)).cuda()
    assert 0 < int(named.sum()) < nbr.shape[0]
    try:
        L.call("mgar_spconv_set_register_gather", register_gather)
        for relu in (1, 0):
            got = (affine_bf16 if bf16 else affine_fp32)(nbr_d, x_d, w_d, 0, sc_d, sh_d, relu)
            nan = torch.isnan(got)
            assert nan[named].all() and not nan[~named].any(), relu
            if relu:
                rest = got[~named].float()
                assert (rest >= 0).all() and not torch.signbit(rest).any() and (rest == 0).any()
    finally:
        L.call("mgar_spconv_set_register_gather", 1)


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------
class _CallLog:
    """Names of the library entry points reached while it is active (the calls go through)."""

    def __init__(self, monkeypatch):
        from multimodal_gar_amd import _lib as L
        self.names = []
        inner = L.call

        def call(name, *args):
            self.names.append(name)
            return inner(name, *args)
        monkeypatch.setattr(L, "call", call)

    def count(self, name):
        return self.names.count(name)

    def clear(self):
        del self.names[:]


def _block(gname, cin, cout, seed, bias=False, relu=True):
    """SparseSequential(conv, BatchNorm1d [, ReLU]).eval() with seeded weights and running statistics away from (0, 1)"""
    from multimodal_gar_amd.pcdet.utils.spconv_utils import spconv
    subm, kernel, stride, padding = C.GEOMETRIES[gname]
    cls = spconv.SubMConv3d if subm else spconv.SparseConv3d
    conv = cls(cin, cout, kernel, stride=stride, padding=padding, bias=bias, indice_key="t")
    bn = nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)
    rng = np.random.default_rng(seed)
    K = int(np.prod(C.triple(kernel)))
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(C.weights(rng, K, cin, cout)).reshape(*C.triple(kernel), cin, cout).permute(4, 0, 1, 2, 3))
        if bias:
            conv.bias.copy_(torch.from_numpy(rng.standard_normal(cout).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(cout).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.3, 3.0, cout).astype(np.float32)))
        bn.weight.copy_(torch.from_numpy(rng.standard_normal(cout).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.standard_normal(cout).astype(np.float32)))
    return spconv.SparseSequential(*([conv, bn] + ([nn.ReLU()] if relu else []))).cuda().eval()


def _sparse_input(cin, bf16, seed=71):
    from multimodal_gar_amd.pcdet.utils.spconv_utils import spconv
    coords, shape, batch = C.geometry_inputs()["faces"]
    x = B.to_bf16(C.wide_range(np.random.default_rng(seed), (coords.shape[0], cin)))
    feats = dev(x).to(BF) if bf16 else dev(x)
    return lambda: spconv.SparseConvTensor(feats, dev(coords), shape, batch), x


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("gname,bias,relu", [("subm_k3", False, True), ("k3_s2_p1", True, True), ("k311_s211_p0", False, False)])
def test_sequential_is_the_new_entry_point_on_fold_bns_tensors(gname, bias, relu, bf16, monkeypatch):
    """SparseSequential(conv, BatchNorm1d [, ReLU]).eval() under no_grad: ONE call of the affine entry point, bit-equal to calling
    it directly with fold_bn's tensors; within the op-level bound of the float64 reference; close to the unfused modules."""
    from multimodal_gar_amd import sparse_ops
    monkeypatch.setattr(sparse_ops, "SPCONV_FOLD_BN", True)
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    log = _CallLog(monkeypatch)
    seq = _block(gname, 32, 64, 80, bias=bias, relu=relu)
    make, x = _sparse_input(32, bf16)
    inp = make()
    with torch.no_grad():
        out = seq(inp)
    name = "mgar_spconv_bf16_fwd_affine" if bf16 else "mgar_spconv_gather_gemm_affine"
    assert log.count(name) == 1 and not [n for n in log.names if n.startswith("mgar_bn") or n in ("mgar_spconv_gather_gemm", "mgar_spconv_bf16_fwd")]
    assert out.features.dtype == (BF if bf16 else torch.float32)
    rb = inp.indice_dict["t"]
    scale, shift = sparse_ops.fold_bn(seq[1], seq[0].bias)
    assert scale.is_cuda and scale.dtype == torch.float32
    K = rb.nbr.shape[1]
    w_d = seq[0].weight.detach().permute(1, 2, 3, 4, 0).reshape(K, 32, 64).contiguous()
    direct = (affine_bf16 if bf16 else affine_fp32)(rb.nbr, inp.features, w_d, 0, scale, shift, int(relu))
    assert torch.equal(bits(out.features), bits(direct))
    w = host(w_d)
    z, S, n = C.gather_gemm_ref(rb.nbr.cpu().numpy(), x, B.to_bf16(w) if bf16 else w)
    check("sequential %s %s" % (gname, "bf16" if bf16 else "fp32"), out.features, z, S, n, host(scale), host(shift), relu, bf16)
    # a second forward computes nothing for the fold
    cached = sparse_ops.fold_bn(seq[1], seq[0].bias)
    assert cached[0] is scale and cached[1] is shift
    # the unfused modules (switch off): the same indices, the same values to rounding
    monkeypatch.setattr(sparse_ops, "SPCONV_FOLD_BN", False)
    log.clear()
    with torch.no_grad():
        off = seq(make())
    assert log.count(name) == 0 and torch.equal(off.indices, out.indices)
    err = (out.features.double() - off.features.double()).abs().max().item()
    scale_of = off.features.double().abs().max().item()
    tol = 2.0 ** -6 if bf16 else PARITY                     # bf16: three roundings against one, a few units in the last place
    record_error("sequential %s fused vs unfused %s" % (gname, "bf16" if bf16 else "fp32"), err, scale_of, tol)
    assert err <= tol * scale_of, (err, scale_of)


def test_launch_counts_and_the_unfused_cases(monkeypatch):
    """With kernel timing on, a fused block credits one spconv launch and no BatchNorm kernel.  The same block in train mode, or
    with a required gradient, or on a BatchNorm without running statistics, is bit-equal to the switch-off run."""
    from multimodal_gar_amd import _lib as L, sparse_ops
    monkeypatch.setattr(sparse_ops, "SPCONV_FOLD_BN", True)
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    seq = _block("subm_k3", 32, 64, 81)
    for bf16, row in ((False, "spconv_gemm"), (True, "spconv_bf16_kernel")):
        make, _ = _sparse_input(32, bf16)
        with torch.no_grad():
            seq(make())                                     # rulebook kernels and the fold happen here, untimed
        L.kernel_timers(True)
        try:
            L.kernel_timers()
            inp = make()
            inp.indice_dict["t"] = sparse_ops.Rulebook(inp.indices, inp.spatial_shape, inp.batch_size, 3, 1, 1, True)
            L.kernel_timers()                               # reset: the rulebook's launches are not the block's
            with torch.no_grad():
                seq(inp)
            torch.cuda.synchronize()
            rows = L.kernel_timers()
        finally:
            L.kernel_timers(False)
        assert rows[row][1] == 1, rows
        assert not [k for k in rows if k.startswith("bn_")] and sum(v[1] for k, v in rows.items() if k.startswith("spconv_")) == 1, rows

    def run(module, grad, fold):
        monkeypatch.setattr(sparse_ops, "SPCONV_FOLD_BN", fold)
        make, _ = _sparse_input(32, False)
        with (torch.enable_grad() if grad else torch.no_grad()):
            return module(make()).features.detach()

    variants = {"train": (copy.deepcopy(seq).train(), False), "grad": (copy.deepcopy(seq), True)}
    no_stats = copy.deepcopy(seq)
    no_stats._modules["1"] = nn.BatchNorm1d(64, eps=1e-3, track_running_stats=False).cuda().eval()
    variants["no running statistics"] = (no_stats, False)
    for what, (module, grad) in variants.items():
        on = run(copy.deepcopy(module), grad, True)
        off = run(copy.deepcopy(module), grad, False)
        assert torch.equal(bits(on), bits(off)), what
    fused, unfused = run(seq, False, True), run(seq, False, False)
    assert not torch.equal(fused, run(copy.deepcopy(seq).train(), False, True))           # train mode really is another function
    assert (fused - unfused).abs().max().item() <= PARITY * unfused.abs().max().item()


# ---- the trunk ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("x_conv1", "x_conv2", "x_conv3", "x_conv4", "encoded")


def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-300)).item()


def _blocks(net):
    """the 12 (conv, BatchNorm1d, ReLU) groups of VoxelBackBone8x in forward order"""
    out = [("conv_input", net.conv_input), ("conv1.0", net.conv1[0])]
    for stage in ("conv2", "conv3", "conv4"):
        out += [("%s.%d" % (stage, i), getattr(net, stage)[i]) for i in range(3)]
    return out + [("conv_out", net.conv_out)]


def _run_trunk(net, data, autocast, fold, record=False):
    """-> {output name: (features, indices)}, {block name: its input SparseConvTensor} if record"""
    from multimodal_gar_amd import sparse_ops
    seen, hooks = {}, []
    if record:
        for name, blk in _blocks(net):
            hooks.append(blk.register_forward_pre_hook(lambda m, args, name=name: seen.__setitem__(name, args[0])))
    saved = sparse_ops.SPCONV_FOLD_BN
    try:
        sparse_ops.SPCONV_FOLD_BN = fold
        with torch.no_grad(), torch.autocast("cuda", dtype=BF, enabled=autocast):
            out = net(dict(data))
    finally:
        sparse_ops.SPCONV_FOLD_BN = saved
        for h in hooks:
            h.remove()
    res = {k: (v.features, v.indices) for k, v in out["multi_scale_3d_features"].items()}
    res["encoded"] = (out["encoded_spconv_tensor"].features, out["encoded_spconv_tensor"].indices)
    return res, seen


@pytest.fixture(scope="module")
def trunk():
    """VoxelBackBone8x on grid [32, 32, 40] in eval mode, 1 500 voxels in 2 samples.  Running statistics: the batch statistics of
    this input (one train-mode pass with momentum 1), then perturbed -- mean moved by up to half a standard deviation, variance
    scaled by 0.6 .. 1.6 -- so the activations stay alive through 12 blocks and the fold matters.  Four runs, shared and left
    unchanged: fp32 unfused (with every block's input), fp32 fused, bf16 autocast fused and unfused."""
    from multimodal_gar_amd import sparse_ops
    from multimodal_gar_amd.pcdet.config import EasyDict
    from multimodal_gar_amd.pcdet.models.backbones_3d import VoxelBackBone8x
    net = fill_deterministic(VoxelBackBone8x(EasyDict(NAME="VoxelBackBone8x"), 4, [32, 32, 40]), seed=5).cuda()
    rng = np.random.default_rng(17)
    cells = rng.choice(2 * 41 * 32 * 32, 1500, replace=False)
    b, z, y, x = np.unravel_index(cells, (2, 41, 32, 32))
    coords = dev(np.stack([b, z, y, x], 1).astype(np.int32))
    feats = dev((rng.standard_normal((1500, 4)) * [12.0, 12.0, 1.5, 0.3] + [20.0, 0.0, -1.0, 0.5]).astype(np.float32))
    data = {"batch_size": 2, "voxel_features": feats, "voxel_coords": coords}
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm1d)]
    assert len(bns) == 12
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad():
        net(dict(data))
    g = torch.Generator().manual_seed(23)
    for m in bns:
        m.momentum = 0.01
        with torch.no_grad():
            std = m.running_var.sqrt()
            m.running_mean.add_(std * (torch.rand(m.num_features, generator=g).cuda() - 0.5))
            m.running_var.mul_(0.6 + torch.rand(m.num_features, generator=g).cuda())
    net.eval()
    saved = sparse_ops.SPCONV_BF16
    try:
        sparse_ops.SPCONV_BF16 = True
        off32, block_in = _run_trunk(net, data, False, False, record=True)
        on32, _ = _run_trunk(net, data, False, True)
        on16, _ = _run_trunk(net, data, True, True)
        off16, _ = _run_trunk(net, data, True, False)
    finally:
        sparse_ops.SPCONV_BF16 = saved
    torch.cuda.synchronize()
    return {"net": net, "data": data, "off32": off32, "on32": on32, "on16": on16, "off16": off16, "block_in": block_in}


def test_trunk_fp32_every_block_on_the_unfused_runs_input(trunk, monkeypatch):
    """Each of the 12 blocks, fused, on the input the unfused run fed it: one affine launch, held to the op-level fp32 bound
    against float64 on the rulebook's own table."""
    from multimodal_gar_amd import sparse_ops
    monkeypatch.setattr(sparse_ops, "SPCONV_FOLD_BN", True)
    log = _CallLog(monkeypatch)
    net = trunk["net"]
    assert len(trunk["block_in"]) == 12
    for name, blk in _blocks(net):
        inp = trunk["block_in"][name]
        assert inp.features.dtype == torch.float32
        log.clear()
        with torch.no_grad():
            out = blk(inp)
        assert log.count("mgar_spconv_gather_gemm_affine") == 1 and log.count("mgar_spconv_gather_gemm") == 0, (name, log.names)
        conv, bn = blk[0], blk[1]
        nbr = inp.indice_dict[conv.indice_key].nbr.cpu().numpy()
        assert nbr.shape[0] == out.features.shape[0]
        K = nbr.shape[1]
        w = host(conv.weight.permute(1, 2, 3, 4, 0).reshape(K, conv.in_channels, conv.out_channels))
        z, S, n = C.gather_gemm_ref(nbr, host(inp.features), w)
        scale, shift = sparse_ops.fold_bn(bn)
        assert not torch.equal(scale, torch.ones_like(scale)) and shift.abs().max() > 0
        check("trunk block %s" % name, out.features, z, S, n, host(scale), host(shift), 1, False)
        assert (out.features > 0).float().mean().item() > 0.05, name                      # the block is alive


def test_trunk_fp32_end_to_end_matches_the_unfused_run(trunk):
    for k in OUTPUTS:
        (a, ai), (b, bi) = trunk["on32"][k], trunk["off32"][k]
        assert a.dtype == b.dtype == torch.float32 and torch.equal(ai, bi) and a.shape[0] >= 32
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        print("%s: fused vs unfused max err %.3e, scale %.3e" % (k, err, scale))
        record_error("voxel trunk eval %s fused vs unfused" % k, err, scale, PARITY)
        assert scale > 0 and torch.isfinite(a).all()
        assert err <= PARITY * scale, (k, err, scale)


def test_trunk_bf16_autocast_fused_is_no_further_from_fp32_than_the_unfused_run(trunk):
    """Indices identical to the fp32 run; for each of the five outputs the fused bf16 run's relative rms distance to the fp32 fused
    run is at most 1.1 x the unfused bf16 run's (the behaviour before the fold: three roundings per block instead of one)."""
    for k in OUTPUTS:
        ref, ri = trunk["on32"][k]
        (a, ai), (b, bi) = trunk["on16"][k], trunk["off16"][k]
        assert a.dtype == BF and torch.equal(ai, ri) and torch.equal(bi, ri), k
        assert torch.isfinite(a.float()).all()
        d_on, d_off = _rel_rms(a, ref), _rel_rms(b, ref)
        print("%s: bf16 fused vs fp32 rel rms %.3e, bf16 unfused %.3e, ratio %.3f" % (k, d_on, d_off, d_on / d_off))
        record_error("voxel trunk eval %s bf16 fused/unfused distance" % k, d_on, d_off, 1.1)
        assert d_off > 0
        assert d_on <= 1.1 * d_off, (k, d_on, d_off)


def test_trunk_launches_per_forward(trunk, monkeypatch):
    """12 convolutions: fp32 -- 12 affine launches; bf16 autocast -- conv_input on the fp32 entry, 11 on the bf16 entry; no plain
    convolution entry and no BatchNorm entry in either."""
    from multimodal_gar_amd import sparse_ops
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    log = _CallLog(monkeypatch)
    for autocast, want in ((False, {"mgar_spconv_gather_gemm_affine": 12}), (True, {"mgar_spconv_gather_gemm_affine": 1, "mgar_spconv_bf16_fwd_affine": 11})):
        log.clear()
        _run_trunk(trunk["net"], trunk["data"], autocast, True)
        got = {n: log.count(n) for n in set(log.names) if n.startswith("mgar_spconv_gather") or n.startswith("mgar_spconv_bf16_fwd") or n.startswith("mgar_bn")}
        assert got == want, got
