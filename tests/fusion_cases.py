"""Case tables and seeded inputs of the op-level tests of the fusion head's three kernels (csrc/gatv2.hip, csrc/dafm.hip,
csrc/roi_align.hip), shared by tests/test_fusion_ops_cpu.py -- which checks, with no kernel involved, the float64
references against the oracle and the conditions the device test relies on -- and tests/test_fusion_edges_gpu.py.

Every case names the code path it is there for.  Graphs are (2, E) int64 tensors [source; target]; RoI inputs are fp32
numpy; DAFM inputs are fp32 torch tensors on the CPU."""
import math

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ GATv2
# One wave per (node, head), 4 waves per block; lanes along C (C / 64 channels per lane: CPL 1, 2, 4, 8, 16); the softmax
# denominator is a lane-strided loop over the incoming edges (one trip per 64 of in-degree).
GAT_CASES = {
    # id: n, H, C, graph, module / mode options
    "n5_tail": dict(n=5, H=1, C=64, graph="complete"),                      # 5 waves in 2 blocks: the tail guard
    "n70_two_trips": dict(n=70, H=3, C=64, graph="complete"),               # in-degree 70: 2 trips; 210 waves
    "n130_three_trips_cpl4": dict(n=130, H=1, C=256, graph="complete"),     # in-degree 130: 3 trips; CPL 4
    "n3_cpl16": dict(n=3, H=1, C=1024, graph="complete"),                   # CPL 16
    "sparse_dups_eval": dict(n=40, H=2, C=128, graph="sparse_dups"),        # directed, shuffled, duplicates, input loops
    "sparse_train": dict(n=40, H=2, C=128, graph="sparse", train=True),     # dropout scale on a sparse graph
    "no_self_loops": dict(n=12, H=2, C=64, graph="holes", add_self_loops=False),   # e0 == e1, empty source ranges
    "shared_concat_nobias": dict(n=9, H=4, C=128, graph="complete", share_weights=True, concat=True, bias=False),
}
GAT_SATURATED = dict(n=70, H=3, C=64, graph="complete", x_scale=30.0)       # logits in the hundreds
SPARSE_SILENT_SOURCES = (3, 17, 29)        # no outgoing edge except, for 3, an input self loop
SPARSE_INPUT_LOOPS = (0, 3, 8, 21)
HOLES_NO_INCOMING = (2, 5, 11)
HOLES_NO_OUTGOING = (0, 5)


def complete_graph(n):
    comb = torch.combinations(torch.arange(n), r=2)
    return torch.cat((comb, torch.flip(comb, [1])), 0).T.contiguous()


def sparse_graph(n=40, p=0.15, seed=11, duplicates=True):
    """Random directed graph, edge list shuffled; SPARSE_SILENT_SOURCES have no outgoing non-loop edge,
    SPARSE_INPUT_LOOPS carry a self loop in the input; with `duplicates`, 25 edges appear twice and 5 of those thrice."""
    rng = np.random.default_rng(seed)
    adj = rng.random((n, n)) < p                       # adj[j, i]: j -> i
    np.fill_diagonal(adj, False)
    adj[list(SPARSE_SILENT_SOURCES), :] = False
    src, dst = np.nonzero(adj)
    src = np.concatenate([src, SPARSE_INPUT_LOOPS]); dst = np.concatenate([dst, SPARSE_INPUT_LOOPS])
    pick = rng.permutation(len(src) - len(SPARSE_INPUT_LOOPS))[:25]
    if duplicates:
        src = np.concatenate([src, src[pick], src[pick[:5]]]); dst = np.concatenate([dst, dst[pick], dst[pick[:5]]])
    order = rng.permutation(len(src))
    return torch.from_numpy(np.stack([src[order], dst[order]]).astype(np.int64))


def holes_graph(n=12, p=0.35, seed=5):
    """For add_self_loops=False: HOLES_NO_INCOMING have no incoming edge, HOLES_NO_OUTGOING no outgoing one (node 5 is
    isolated); node 7 keeps an input self loop, which is then an ordinary edge.  Every other target has an incoming edge."""
    rng = np.random.default_rng(seed)
    adj = rng.random((n, n)) < p
    np.fill_diagonal(adj, False)
    adj[7, 7] = True
    adj[:, list(HOLES_NO_INCOMING)] = False
    adj[list(HOLES_NO_OUTGOING), :] = False
    for i in range(n):
        if i not in HOLES_NO_INCOMING and not adj[:, i].any():
            adj[(i + 1) % n if (i + 1) % n not in HOLES_NO_OUTGOING else (i + 2) % n, i] = True
    src, dst = np.nonzero(adj)
    order = rng.permutation(len(src))
    return torch.from_numpy(np.stack([src[order], dst[order]]).astype(np.int64))


def gat_graph(kind, n):
    if kind == "complete":
        return complete_graph(n)
    if kind == "sparse_dups":
        return sparse_graph(n, duplicates=True)
    if kind == "sparse":
        return sparse_graph(n, duplicates=False)
    if kind == "holes":
        return holes_graph(n)
    raise KeyError(kind)


def random_graph(n, e, seed, loops=True):
    """Property-test input: e directed edges drawn with replacement (duplicates, self loops when `loops`), unsorted."""
    rng = np.random.default_rng(seed)
    if n == 0 or e == 0:
        return torch.zeros((2, 0), dtype=torch.int64)
    src = rng.integers(0, n, e); dst = rng.integers(0, n, e)
    if not loops:
        dst = np.where(dst == src, (dst + 1) % n, dst)
    if n > 4:                                           # isolated nodes: nothing into or out of the last two
        keep = (src < n - 2) & (dst < n - 2)
        src, dst = src[keep], dst[keep]
    return torch.from_numpy(np.stack([src, dst]).astype(np.int64))


# ------------------------------------------------------------------------------------------------ DAFM
# One wave per row, 4 per block; lanes along j hold MGAR_DAFM_MAX_N / 64 = 2 columns each; lanes along d step 256 floats.
DAFM_CASES = {
    "n1_n64_n65_D64": dict(counts=[1, 64, 65, 2], D=64),           # n = 1; second column register starts; 16 lanes along d
    "n128_n127_D192": dict(counts=[128, 127, 3], D=192),           # full capacity; 258 rows (258 % 4 = 2); partial trip along d
    "empty_scenes_D320": dict(counts=[5, 0, 7, 0], D=320),         # duplicate offsets mid / end; partial second trip along d
    "e_underflow": dict(counts=[33], D=512, de_max=2000.0),        # E underflows to exact zeros in fp32: logits 0 there
    "large_logits": dict(counts=[33], D=512, qk_scale=4.0),        # large logits through __expf
}
DAFM_SIGMA = 10.0


def dafm_inputs(counts, D, de_max=20.0, qk_scale=1.0, seed=1):
    g = torch.Generator().manual_seed(seed)
    rows = sum(counts)
    q = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    k = torch.randn(rows, D, generator=g) * 0.5 * qk_scale
    v = torch.randn(rows, D, generator=g)
    des = []
    for n in counts:
        d = torch.rand(n, n, generator=g) * de_max
        d.fill_diagonal_(0)
        des.append(d)
    grad = torch.randn(rows, D, generator=g)
    return q, k, v, des, grad


# ------------------------------------------------------------------------------------------------ RoIAlign
CLEARANCE = 1e-3            # asserted for every RoI of every case (test_fusion_ops_cpu.py)
_DRAW_CLEARANCE = 2e-3      # boxes are drawn until they clear this


def _axis_clearance(lo, hi, size, pooled, sampling_ratio, aligned, exact_zero):
    """Distance of one axis of one RoI to the nearest discontinuity of RoIAlign, in float64: a sample coordinate at -1
    or `size` (the sample switches between counted and dropped) or extent / pooled at an integer (ceil changes the sample
    count).  exact_zero: the two box coordinates are the same number, so the extent is 0 in every precision and the
    count is 0 in every precision -- rounding cannot move it, and it has no samples."""
    ext = hi - lo
    if not aligned:
        ext = max(ext, 1.0)
    d = math.inf
    if sampling_ratio > 0:
        g = sampling_ratio
    else:
        t = ext / pooled
        g = math.ceil(t)
        if not exact_zero:
            d = min(t - math.floor(t), math.ceil(t) - t)
    b = ext / pooled
    for p in range(pooled):
        for i in range(g):
            c = lo + p * b + (i + 0.5) * b / g
            d = min(d, abs(c + 1.0), abs(c - size))
    return d


def roi_clearance(rois, H, W, out_size, scale, sampling_ratio=-1, aligned=False):
    """(K,) float64: each RoI's smallest distance to a discontinuity (see _axis_clearance)."""
    ph, pw = (out_size, out_size) if isinstance(out_size, int) else out_size
    off = 0.5 if aligned else 0.0
    out = np.empty(len(rois))
    for k, r in enumerate(np.asarray(rois)):
        x1, y1, x2, y2 = [float(v) * scale - off for v in r[1:]]
        out[k] = min(_axis_clearance(x1, x2, W, pw, sampling_ratio, aligned, aligned and r[1] == r[3]),
                     _axis_clearance(y1, y2, H, ph, sampling_ratio, aligned, aligned and r[2] == r[4]))
    return out


def _draw_boxes(rng, count, n_img, H, W, out_size, scale, sampling_ratio=-1, aligned=False, margin=0.3):
    """`count` random boxes [batch, x1, y1, x2, y2] (fp32), many reaching outside the image, each drawn again until it
    clears _DRAW_CLEARANCE (a fixed seed makes the accepted sequence reproducible)."""
    wpx, hpx = W / scale, H / scale
    out = []
    while len(out) < count:
        x1 = rng.uniform(-margin * wpx, 0.9 * wpx); y1 = rng.uniform(-margin * hpx, 0.9 * hpx)
        w = rng.uniform(0.05 * wpx, 0.9 * wpx); h = rng.uniform(0.05 * hpx, 0.9 * hpx)
        box = np.array([[rng.integers(0, n_img), x1, y1, x1 + w, y1 + h]], np.float32)
        if roi_clearance(box, H, W, out_size, scale, sampling_ratio, aligned)[0] >= _DRAW_CLEARANCE:
            out.append(box[0])
    return np.stack(out)


def _roi_case(feat_shape, rois, out_size, scale, sampling_ratio=-1, aligned=False, seed=0):
    feat = np.random.default_rng(seed).standard_normal(feat_shape).astype(np.float32)
    return dict(feat=feat, rois=np.ascontiguousarray(rois, np.float32), out_size=out_size, scale=scale,
                sampling_ratio=sampling_ratio, aligned=aligned)


def roi_grid_stride():
    """K * C * 5 * 5 = 4 201 600 outputs: 7 296 above the 16384 x 256 launch cap, so the grid-stride loop takes a second
    trip.  150 random boxes (many partly outside the image) and 52 all-zero padded boxes, as the model pads to 100 per
    image."""
    rng = np.random.default_rng(2024)
    boxes = _draw_boxes(rng, 150, 2, 6, 10, 5, 1 / 16.0)
    pad = np.zeros((52, 5), np.float32); pad[26:, 0] = 1
    rois = np.concatenate([boxes[:75], pad[:26], boxes[75:], pad[26:]])
    return _roi_case((2, 832, 6, 10), rois, 5, 1 / 16.0, seed=1)


def roi_non_square(out_size, sampling_ratio=-1):
    """PH != PW on a batch of 3 with RoIs on the last image (and the others)."""
    rng = np.random.default_rng(7)
    rois = _draw_boxes(rng, 7, 3, 9, 13, out_size, 1 / 16.0, sampling_ratio)
    rois[:3, 0] = 2; rois[3, 0] = 0; rois[4, 0] = 1
    return _roi_case((3, 6, 9, 13), rois, out_size, 1 / 16.0, sampling_ratio, seed=2)


def roi_contended():
    """64 copies of one box + 64 random boxes on one small map: the backward's atomics contend on the same addresses."""
    rng = np.random.default_rng(9)
    boxes = _draw_boxes(rng, 65, 1, 9, 14, 5, 1 / 16.0)
    rois = np.concatenate([np.repeat(boxes[:1], 64, 0), boxes[1:]])
    return _roi_case((1, 4, 9, 14), rois, 5, 1 / 16.0, seed=3)


ROI_DEGENERATE_ZERO_OUTPUT = (0, 1, 2, 3, 4)      # rows of roi_degenerate() without any counted sample


def roi_degenerate():
    """aligned=True.  Rows: 0 inverted in x and y, 1 inverted in x only, 2 zero area (x2 == x1 and y2 == y1 as numbers: the
    extent is exactly 0 in any precision), 3 entirely beyond -1, 4 entirely beyond the far edge, 5 an ordinary box.  The
    scale is a power of two, so box * scale is exact in fp32.  Rows 0-4 have no counted sample: their output is 0."""
    rois = np.array([[0, 100.0, 80.0, 40.0, 30.0],
                     [1, 120.0, 20.0, 50.0, 90.0],
                     [0, 64.0, 40.0, 64.0, 40.0],
                     [1, -90.0, -80.0, -30.0, -28.0],
                     [0, 250.0, 170.0, 300.0, 200.0],
                     [1, 21.0, 13.0, 150.0, 110.0]], np.float32)
    return _roi_case((2, 3, 9, 14), rois, 3, 1 / 16.0, aligned=True, seed=4)


ROI_CASES = {
    "grid_stride": roi_grid_stride,
    "non_square_3x7": lambda: roi_non_square((3, 7)),
    "non_square_7x3": lambda: roi_non_square((7, 3)),
    "non_square_3x7_sr3": lambda: roi_non_square((3, 7), 3),
    "non_square_7x3_sr3": lambda: roi_non_square((7, 3), 3),
    "contended": roi_contended,
    "degenerate_aligned": roi_degenerate,
}
