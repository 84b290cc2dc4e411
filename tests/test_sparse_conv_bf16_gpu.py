"""csrc/sparse_conv_bf16.hip on the device: the forward gather-GEMM of the sparse convolution for bf16 rows (bf16 MFMA) against
the float64 reference of tests/sparse_conv_cases.py on the ROUNDED operands, the host routing around it, the bf16 row-major
BatchNorm, and the Voxel R-CNN trunk / voxel route in bf16 against their fp32 runs.

Every value is compared per ELEMENT with the bound of tests/sparse_conv_bf16_cases.py (fp32 accumulation of exact products in
any order + one bf16 rounding; pinned as satisfiable by tests/test_sparse_conv_bf16_cpu.py); a row without a product must be an
exact zero; two launches must agree bit for bit.  `record_error` logs the share of the bound each comparison used."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import sparse_conv_bf16_cases as B
import sparse_conv_cases as C
from conftest import record_error

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from param_fill import fill_deterministic  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# The project's tolerances of the bf16 configurations, as stated (and derived) in tests/test_bf16_gpu.py: one stage fed the fp32
# run's own inputs rounded to bf16 / the 16 final outputs of a randomly initialised network, both as relative rms.
BF16_STAGE_RMS = 1.5e-2
BF16_E2E_RMS = 0.5

TRUNK_GEOMETRIES = ("subm_k3", "k3_s2_p1", "k3_s2_p011", "k311_s211_p0")          # the four layer geometries of VoxelBackBone8x
BLOCKS_AFTER_CONV_INPUT = 11                                                       # conv1 1 + conv2..4 3 each + conv_out 1


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared tables are read-only


def host(t):
    return t.detach().float().cpu().numpy()


def bf16_fwd(nbr_d, x_bf, w_d, flip=0):
    """mgar_spconv_bf16_fwd called by name: x_bf (Ni, Cin) bf16, w_d (K, Cin, Cout) fp32 -> (No, Cout) bf16"""
    from multimodal_gar_amd import _lib as L
    K, cin, cout = w_d.shape
    n_out = nbr_d.shape[0]
    nbytes = L.raw("mgar_spconv_bf16_workspace_bytes", K, cin, cout)
    assert nbytes == K * (cin // 16) * -(-cout // 32) * 1024
    packed = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    out = torch.full((n_out, cout), float("nan"), dtype=BF, device="cuda")          # "fully written": no NaN may survive
    L.call("mgar_spconv_bf16_fwd", n_out, K, cin, cout, L.pptr(x_bf, BF), L.iptr(nbr_d), L.fptr(w_d), int(flip),
           L.dev_ptr(packed, torch.uint8), L.pptr(out, BF), L.stream_of(x_bf))
    return out


def check(what, got, ref, S, n):
    got = host(got).astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    ratio = np.abs(got - ref) / B.bound(ref, S, n)
    used = float(ratio.max()) if ratio.size else 0.0
    record_error(what, used, 1.0, 1.0)
    print("%s: err / bound %.3g" % (what, used))
    assert used <= 1.0, "%s: err / bound %.3g at %s" % (what, used, np.unravel_index(ratio.argmax(), ratio.shape))
    assert (got[n[:, 0] == 0] == 0).all(), "%s: a row without a neighbour is not an exact zero" % what


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.value_cases()))
def test_kernel_against_float64_on_the_rounded_operands(name):
    """Channel plans at 193 rows and K = 27 (the trunk's six, 128 x 128, C_in not a power of two, C_out = 1 and 33), row counts
    1 .. 1 025 across the 32-row wave and the 128-row workgroup tile, K = 1, 2, 3, 8 with an empty and a full column, mirrored
    offsets, whole 64-row tiles without a neighbour (exact zeros), the 8 200 x 27 main table; wide_range features.  Two
    launches give identical bits."""
    nbr, x, w, flip = B.operands(name)
    ref, S, n = C.gather_gemm_ref(nbr, x, w, flip)
    nbr_d, x_d, w_d = dev(nbr), dev(x).to(BF), dev(w)
    assert np.array_equal(host(x_d), x)                                            # the rounding was done by torch already
    got = bf16_fwd(nbr_d, x_d, w_d, flip)
    assert got.dtype == BF
    check(name, got, ref, S, n)
    assert torch.equal(got.view(torch.int16), bf16_fwd(nbr_d, x_d, w_d, flip).view(torch.int16))
    if name.startswith("alternate_tiles"):
        empty = (np.arange(nbr.shape[0]) // 64) % 2 == 1
        assert empty.any() and (host(got)[empty] == 0).all()


@pytest.mark.parametrize("cin,cout", B.ROWS_PLANS)
def test_a_rows_bits_do_not_depend_on_its_position_or_on_the_launch_size(cin, cout):
    """Row o of the 1 025-row launch == the same table row launched alone == the same table row at another position (a permuted
    table), bit for bit."""
    nbr, x, w, flip = B.operands("rows_1025_%dx%d" % (cin, cout))
    x_d, w_d = dev(x).to(BF), dev(w)
    full = bf16_fwd(dev(nbr), x_d, w_d).view(torch.int16)
    perm = np.random.default_rng(11).permutation(nbr.shape[0])
    assert (perm != np.arange(len(perm))).sum() > 1000
    moved = bf16_fwd(dev(nbr[perm]), x_d, w_d).view(torch.int16)
    assert torch.equal(moved, full[torch.from_numpy(perm).cuda()])
    for o in (0, 1, 31, 32, 63, 127, 128, 640, 1023, 1024):
        alone = bf16_fwd(dev(nbr[o:o + 1]), x_d, w_d).view(torch.int16)
        assert torch.equal(alone[0], full[o]), o


# ---- the wrappers -------------------------------------------------------------------------------------------------------------
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


def _layer(gname, cin, cout, seed):
    from multimodal_gar_amd.pcdet.utils.spconv_utils import spconv
    subm, kernel, stride, padding = C.GEOMETRIES[gname]
    cls = spconv.SubMConv3d if subm else spconv.SparseConv3d
    m = cls(cin, cout, kernel, stride=stride, padding=padding, bias=False, indice_key="t").cuda()
    K = int(np.prod(C.triple(kernel)))
    w = C.weights(np.random.default_rng(seed), K, cin, cout)                       # (K, Cin, Cout)
    with torch.no_grad():
        m.weight.copy_(dev(w).reshape(*C.triple(kernel), cin, cout).permute(4, 0, 1, 2, 3))
    return m, w


@pytest.mark.parametrize("gname", TRUNK_GEOMETRIES)
def test_wrapper_routing(gname, monkeypatch):
    from multimodal_gar_amd import sparse_ops
    from multimodal_gar_amd.pcdet.utils.spconv_utils import spconv
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    log = _CallLog(monkeypatch)
    coords, shape, batch = C.geometry_inputs()["faces"]
    subm, kernel, stride, padding = C.GEOMETRIES[gname]
    oidx, oshape, nbr, _ = C.rulebook_ref(coords, shape, kernel, stride, padding, subm)
    assert nbr.shape[0] > 20
    coords_d = dev(coords)

    def run(module, feats):
        log.clear()
        with torch.no_grad():
            out = module(spconv.SparseConvTensor(feats, coords_d, shape, batch))
        assert np.array_equal(out.indices.cpu().numpy().reshape(-1, 4), oidx) and list(out.spatial_shape) == oshape
        return out.features

    m, w = _layer(gname, 32, 64, 70)
    x = B.to_bf16(C.wide_range(np.random.default_rng(71), (coords.shape[0], 32)))
    x_bf = dev(x).to(BF)
    # bf16 features: the new entry point, bf16 out, within the bound of the float64 reference on the reference's table
    got = run(m, x_bf)
    assert got.dtype == BF and log.count("mgar_spconv_bf16_fwd") == 1 and log.count("mgar_spconv_gather_gemm") == 0
    ref, S, n = C.gather_gemm_ref(nbr, x, B.to_bf16(w))
    check("wrapper %s bf16" % gname, got, ref, S, n)
    # fp32 features: today's path, bit for bit a direct mgar_spconv_gather_gemm call
    got32 = run(m, dev(x))
    assert got32.dtype == torch.float32 and log.count("mgar_spconv_bf16_fwd") == 0 and log.count("mgar_spconv_gather_gemm") == 1
    K = nbr.shape[1]
    direct = sparse_ops._gather_gemm(nbr.shape[0], K, 32, 64, dev(x), dev(nbr), dev(w), 0)
    assert torch.equal(got32, direct)
    # the switch off: bf16 features are widened as before
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", False)
    off = run(m, x_bf)
    assert off.dtype == torch.float32 and log.count("mgar_spconv_bf16_fwd") == 0 and torch.equal(off, direct)
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    # bf16 features that need a gradient: widened, training stays fp32
    log.clear()
    out = m(spconv.SparseConvTensor(x_bf, coords_d, shape, batch)).features
    assert out.dtype == torch.float32 and out.requires_grad and log.count("mgar_spconv_bf16_fwd") == 0 and torch.equal(out.detach(), direct)
    # an unsupported plan falls back and is still right (fp32 kernel on the widened rows: the fp32 bound of the cases module)
    m2, w2 = _layer(gname, 24, 40, 72)
    x2 = B.to_bf16(C.wide_range(np.random.default_rng(73), (coords.shape[0], 24)))
    got2 = run(m2, dev(x2).to(BF))
    assert log.count("mgar_spconv_bf16_fwd") == 0 and log.count("mgar_spconv_gather_gemm") == 1
    ref2, S2, n2 = C.gather_gemm_ref(nbr, x2, w2)
    used = float((np.abs(host(got2).astype(np.float64) - ref2) / C.bound(n2, 2, S2)).max())
    record_error("wrapper %s fallback 24x40" % gname, used, 1.0, 1.0)
    assert got2.dtype == torch.float32 and used <= 1.0, used


# ---- BatchNorm on bf16 rows ---------------------------------------------------------------------------------------------------
def _within_one_rounding(got, want):
    """elementwise |err| <= 2**-8 |want| + 2e-5 max|want|; returns (ok, worst err / bound) -- the form of test_conv3d_bf16_gpu.py"""
    err = (got.double() - want).abs()
    bound = 2.0 ** -8 * want.abs() + 2e-5 * want.abs().max()
    return bool((err <= bound).all()), (err / bound).max().item()


@pytest.mark.parametrize("rows,c", [(1, 16), (193, 64), (8200, 128)])
def test_bn_act_rows_on_bf16_rows(rows, c):
    """bf16 in and out, statistics and affine fp32, forward only: float64 BatchNorm(train) + ReLU of the bf16 input within one
    bf16 rounding; running statistics bit for bit those of the fp32 kernel on the widened input."""
    from multimodal_gar_amd import bn_ops
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows, c, generator=g) * torch.linspace(0.1, 4.0, c) + torch.linspace(-2.0, 2.0, c)).to(BF).cuda()
    bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, c)); bn.bias.copy_(torch.linspace(-0.3, 0.3, c))
    b16, b32 = copy.deepcopy(bn), copy.deepcopy(bn)
    with torch.no_grad():
        y = bn_ops.bn_act_rows(x, b16, True)
        y32 = bn_ops.bn_act_rows(x.float(), b32, True)
    assert y is not None and y.dtype == BF and y.shape == x.shape and y32.dtype == torch.float32
    xd = x.double()
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    want = torch.relu((xd - mean) / torch.sqrt(var + bn.eps) * bn.weight.double() + bn.bias.double())
    ok, ratio = _within_one_rounding(y, want)
    record_error("bn_act_rows bf16 (%d, %d) err / bound" % (rows, c), ratio, 1.0, 1.0)
    assert ok, ratio
    assert torch.equal(b16.running_mean, b32.running_mean) and torch.equal(b16.running_var, b32.running_var)
    assert b16.num_batches_tracked.item() == b32.num_batches_tracked.item() == 1
    assert not torch.equal(b16.running_mean, bn.running_mean)
    # a bf16 input that needs a gradient, or eval mode: not taken, as before
    assert bn_ops.bn_act_rows(x.clone().requires_grad_(True), copy.deepcopy(bn), True) is None
    assert bn_ops.bn_act_rows(x, copy.deepcopy(bn), True) is None                 # grad enabled, the affine requires grad
    with torch.no_grad():
        assert bn_ops.bn_act_rows(x, copy.deepcopy(bn).eval(), True) is None


# ---- the trunk ----------------------------------------------------------------------------------------------------------------
STAGES = ("conv1", "conv2", "conv3", "conv4", "conv_out")
X_CONVS = ("x_conv1", "x_conv2", "x_conv3", "x_conv4")


def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()


def _run_trunk(net, data, autocast):
    """-> {x_conv1..4, encoded: (features, indices)}, {stage: its input SparseConvTensor}"""
    stage_in, hooks = {}, []
    for name in STAGES:
        hooks.append(getattr(net, name).register_forward_pre_hook(lambda m, args, name=name: stage_in.__setitem__(name, args[0])))
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF, enabled=autocast):
            out = net(dict(data))
    finally:
        for h in hooks:
            h.remove()
    res = {k: (v.features, v.indices) for k, v in out["multi_scale_3d_features"].items()}
    res["encoded"] = (out["encoded_spconv_tensor"].features, out["encoded_spconv_tensor"].indices)
    return res, stage_in


def _emulation(net):
    """The bf16 trunk restated on the fp32 kernels alone (the caller switches the bf16 kernel off): weights of every block after
    conv_input, every convolution output after conv_input and every BatchNorm + ReLU output rounded to bf16 -- the points at which
    the bf16 route rounds.  The two differ in summation order alone."""
    from multimodal_gar_amd.pcdet.utils.spconv_utils import SparseConvolution, SparseSequential
    emu = copy.deepcopy(net)

    def rounded(m, args, out):
        return out.replace_feature(out.features.to(BF).float())
    first = emu.conv_input[0]
    for m in emu.modules():
        if isinstance(m, SparseConvolution) and m is not first:
            m.weight.data = m.weight.data.to(BF).float()
            m.register_forward_hook(rounded)
        if isinstance(m, SparseSequential) and len(m) == 3 and isinstance(m[0], SparseConvolution):
            m.register_forward_hook(rounded)                                       # (conv, BatchNorm1d, ReLU): the block's output
    return emu


@pytest.fixture(scope="module")
def trunk():
    """One fp32 run, one bf16 run and one emulation run of VoxelBackBone8x, shared (and left unchanged) by the tests below."""
    from multimodal_gar_amd import sparse_ops
    from multimodal_gar_amd.pcdet.config import EasyDict
    from multimodal_gar_amd.pcdet.models.backbones_3d import VoxelBackBone8x
    net = fill_deterministic(VoxelBackBone8x(EasyDict(NAME="VoxelBackBone8x"), 4, [32, 32, 40]), seed=5).cuda().train()
    assert net.sparse_shape == [41, 32, 32]
    rng = np.random.default_rng(17)
    cells = rng.choice(2 * 41 * 32 * 32, 1500, replace=False)
    b, z, y, x = np.unravel_index(cells, (2, 41, 32, 32))
    coords = dev(np.stack([b, z, y, x], 1).astype(np.int32))
    feats = dev((rng.standard_normal((1500, 4)) * [12.0, 12.0, 1.5, 0.3] + [20.0, 0.0, -1.0, 0.5]).astype(np.float32))
    data = {"batch_size": 2, "voxel_features": feats, "voxel_coords": coords}
    saved = sparse_ops.SPCONV_BF16
    try:
        sparse_ops.SPCONV_BF16 = True
        r32, in32 = _run_trunk(copy.deepcopy(net), data, False)
        net16 = copy.deepcopy(net)
        r16, _ = _run_trunk(net16, data, True)
        sparse_ops.SPCONV_BF16 = False
        remu, _ = _run_trunk(_emulation(net), data, False)
    finally:
        sparse_ops.SPCONV_BF16 = saved
    torch.cuda.synchronize()
    return {"net": net, "fp32": r32, "bf16": r16, "emulation": remu, "stage_in": in32}


def test_trunk_bf16_indices_identical_and_features_as_close_to_fp32_as_the_emulation(trunk):
    r32, r16, remu = trunk["fp32"], trunk["bf16"], trunk["emulation"]
    for k in X_CONVS + ("encoded",):
        assert r32[k][0].dtype == torch.float32 and r16[k][0].dtype == BF and remu[k][0].dtype == torch.float32
        assert torch.equal(r32[k][1], r16[k][1]) and torch.equal(r32[k][1], remu[k][1]), k
        assert torch.isfinite(r16[k][0].float()).all()
    sites = [r32[k][1].shape[0] for k in X_CONVS]
    print("active sites per level:", sites)
    assert min(sites) >= 100                          # x_conv4 lives on a 2 x (5, 4, 4) grid: at most 160
    for k in X_CONVS:
        d_own, d_emul = _rel_rms(r16[k][0], r32[k][0]), _rel_rms(remu[k][0], r32[k][0])
        print("%s: bf16 trunk vs fp32 rel rms %.3e, emulation on the fp32 kernels %.3e" % (k, d_own, d_emul))
        record_error("voxel trunk %s bf16 vs fp32 (rel rms)" % k, d_own, 1.0, max(1.5 * d_emul, 1e-3))
        record_error("voxel trunk %s emulation vs fp32 (rel rms)" % k, d_emul, 1.0, max(1.5 * d_emul, 1e-3))
        assert d_emul > 0
        assert d_own <= max(1.5 * d_emul, 1e-3), (k, d_own, d_emul)


def test_trunk_stages_on_the_fp32_runs_inputs(trunk, monkeypatch):
    """Every stage of the trunk on the fp32 run's recorded input rounded to bf16: rel rms of its output against the fp32 stage
    output <= BF16_STAGE_RMS, through the new kernel."""
    from multimodal_gar_amd import sparse_ops
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    log = _CallLog(monkeypatch)
    net = copy.deepcopy(trunk["net"])
    want = dict(zip(STAGES, X_CONVS + ("encoded",)))
    for name in STAGES:
        inp = trunk["stage_in"][name]
        assert inp.features.dtype == torch.float32
        log.clear()
        with torch.no_grad():
            out = getattr(net, name)(inp.replace_feature(inp.features.to(BF)))
        blocks = 1 if name in ("conv1", "conv_out") else 3
        assert out.features.dtype == BF and log.count("mgar_spconv_bf16_fwd") == blocks and log.count("mgar_spconv_gather_gemm") == 0
        assert torch.equal(out.indices, trunk["fp32"][want[name]][1])
        err = _rel_rms(out.features, trunk["fp32"][want[name]][0])
        print("stage %s: bf16 rel rms %.3e" % (name, err))
        record_error("voxel trunk stage %s bf16 vs fp32 (rel rms)" % name, err, 1.0, BF16_STAGE_RMS)
        assert err <= BF16_STAGE_RMS, (name, err)


# ---- the voxel route ----------------------------------------------------------------------------------------------------------
class _VoxelQueryRecorder:
    """Every index tensor the voxel query writes during a forward pass, at the hook point of test_bf16_gpu.py's _IndexRecorder:
    the shim module the Python layer calls through (dense-table and hash-table form; idx is the last argument of both)."""
    NAMES = ("voxel_query_wrapper", "voxel_query_hash_wrapper")

    def __init__(self):
        self.log, self._saved = [], []

    def __enter__(self):
        from multimodal_gar_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as sm
        for name in self.NAMES:
            fn = getattr(sm, name)
            self._saved.append((sm, name, fn))

            def wrapped(*args, fn=fn, name=name, **kw):
                r = fn(*args, **kw)
                assert args[-1].dtype == torch.int32
                self.log.append((name, args[-1].detach().clone()))
                return r
            setattr(sm, name, wrapped)
        return self

    def __exit__(self, *exc):
        for mod, name, fn in self._saved:
            setattr(mod, name, fn)


def _no_dropout(module):
    for m in module.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0


def test_voxel_route_bf16_vs_fp32(monkeypatch):
    """ForwardStep(route="voxel") in fp32 and bf16 with the same weights, 1 clip x 2 frames x 4 actors x 4 096 points, 96 x 160
    images, eager: voxel coordinates and voxel-query indices identical, the 16 outputs finite and within BF16_E2E_RMS, and the
    bf16 run's trunk on the new kernel (the fp32 gather-GEMM for conv_input only)."""
    from multimodal_gar_amd import sparse_ops, workload as W
    monkeypatch.setattr(sparse_ops, "SPCONV_BF16", True)
    log = _CallLog(monkeypatch)
    device = torch.device("cuda")
    steps = {}
    for prec in ("fp32", "bf16"):
        steps[prec] = W.ForwardStep(4, 4096, device, route="voxel", precision=prec, seed=9)
        _no_dropout(steps[prec].module)
    fill_deterministic(steps["fp32"].module, seed=9)
    steps["bf16"].module.load_state_dict(steps["fp32"].module.state_dict())        # copy_ keeps each destination's dtype
    batch = W.make_batch(35, 1, 2, 4, 4096, 96, 160, device)
    outs, queries, coords, calls = {}, {}, {}, {}
    for prec in ("fp32", "bf16"):
        bb = steps[prec].module.net.LiDAR_backbone.model.backbone_3d
        seen = []
        hook = bb.register_forward_pre_hook(lambda m, args, seen=seen: seen.append(args[0]["voxel_coords"].detach().clone()))
        log.clear()
        try:
            with _VoxelQueryRecorder() as rec:
                outs[prec] = steps[prec].run_eager(batch)
            torch.cuda.synchronize()
        finally:
            hook.remove()
        queries[prec], coords[prec], calls[prec] = rec.log, seen, list(log.names)
    assert len(coords["fp32"]) == len(coords["bf16"]) >= 1
    for a, b in zip(coords["fp32"], coords["bf16"]):
        assert a.shape[0] > 100 and torch.equal(a, b)
    assert len(queries["fp32"]) == len(queries["bf16"]) >= 1
    for (n1, t1), (n2, t2) in zip(queries["fp32"], queries["bf16"]):
        assert n1 == n2 and torch.equal(t1, t2), "integer output of %s differs between the fp32 and the bf16 run" % n1
    assert len(outs["bf16"]) == len(outs["fp32"]) == 16
    worst = 0.0
    for i, (a, b) in enumerate(zip(outs["bf16"], outs["fp32"])):
        assert a.shape == b.shape and torch.isfinite(a.float()).all() and torch.isfinite(b).all(), i
        worst = max(worst, _rel_rms(a.float(), b))
    print("voxel route: worst end-to-end bf16-vs-fp32 rel rms %.2e" % worst)
    record_error("voxel route bf16 vs fp32 (worst rel rms of 16 outputs)", worst, 1.0, BF16_E2E_RMS)
    assert worst <= BF16_E2E_RMS, worst
    n_trunks = len(coords["bf16"])
    assert calls["fp32"].count("mgar_spconv_bf16_fwd") == 0
    assert calls["fp32"].count("mgar_spconv_gather_gemm") == (BLOCKS_AFTER_CONV_INPUT + 1) * n_trunks
    assert calls["bf16"].count("mgar_spconv_bf16_fwd") == BLOCKS_AFTER_CONV_INPUT * n_trunks       # once per supported block
    assert calls["bf16"].count("mgar_spconv_gather_gemm") == n_trunks                               # conv_input only
