"""Seeded inputs of the op-level Voxel-RoI pooling tests, shared by tests/test_voxel_roi_pool_cpu.py (which checks the
conditions the GPU test relies on -- near-tie share, conditioning ratio -- without any kernel) and
tests/test_voxel_roi_pool_gpu.py.

A case is what `NeighborVoxelSAModuleMSG` hands the fused kernels for one scale: voxel centres `xyz` of a sparsely
occupied (Z, Y, X) grid of 0.25 x 0.25 x 0.5 m cells, continuous random queries, `idx_raw` exactly as the voxel query
writes it (the C oracle's transcription of voxel_query_gpu.cu: hits in scan order, short rows padded with their first hit,
-1 in slot 0 of an empty neighbourhood and nothing else written to that row), random-normal projected features, a
non-trivial position weight and BatchNorm affine.  All arrays are fp32 / int32 numpy; the tests widen or upload them."""
import numpy as np

VOXEL = np.array([0.25, 0.25, 0.5], np.float32)
EMPTY_SHARE = 0.03          # queries moved far outside the grid on top of the naturally empty ones
EPS = 1e-5

# (M, nsample, C): forward / backward / autograd cases
FULL_SIZES = [(180, 16, 16), (2117, 16, 32), (4999, 8, 12), (70000, 16, 16), (333, 1, 1), (130, 255, 5), (5, 1, 3), (1, 1, 2)]
ALL_EMPTY = (64, 8, 8)
CAP_CASE = (270000, 16, 4)  # M * nsample > 2048 blocks * 256 threads * 8: the block count of the moments pass is capped
CONDITIONING = ["translated", "one_sided"]
CONDITIONING_SIZE = (4999, 16, 16)
TRANSLATION = (70.0, -40.0, 0.0)
ONE_SIDED_SHIFT = 4.0       # metres along x: every neighbour lies on one side of its query
NEAR_TIE_MARGIN = 1e-5
NEAR_TIE_CAP = 5e-3         # at most 0.5 % of the non-empty (m, c) entries may be masked


def size_id(size):
    return "M%d_ns%d_C%d" % tuple(size)


def _scan(nsample):
    """(z, y, x) cell range and radius of the query, occupancy of the grid: small neighbourhoods give a mix of full and
    short rows at nsample 8 / 16, the wide one fills 255 slots away from the grid's border."""
    if nsample <= 16:
        return (1, 2, 2), 0.75, 0.30
    return (3, 6, 6), 2.0, 0.60


def make_case(M, nsample, C, seed=0, variant=None):
    """variant: None, "all_empty" (every query far outside), "translated" (all coordinates moved by TRANSLATION before
    they are rounded to fp32) or "one_sided" (queries moved by ONE_SIDED_SHIFT along -x AFTER the query, so that
    |E[r_x]| is several standard deviations of r_x; no query is moved outside the grid)."""
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng([seed, M, nsample, C])
    Z, Y, X = 8, 64, 64
    max_range, radius, occupancy = _scan(nsample)
    lo = np.array([-8.0, -8.0, -2.0], np.float64)
    if variant == "translated":
        lo = lo + np.array(TRANSLATION, np.float64)
    z, y, x = np.nonzero(rng.random((Z, Y, X)) < occupancy)
    perm = rng.permutation(len(z))
    zyx = np.stack([z[perm], y[perm], x[perm]], 1).astype(np.int32)
    n_vox = len(zyx)
    xyz = ((zyx[:, ::-1].astype(np.float64) + 0.5) * VOXEL + lo).astype(np.float32)
    v2p = -np.ones((1, Z, Y, X), np.int32)
    v2p[0, zyx[:, 0], zyx[:, 1], zyx[:, 2]] = np.arange(n_vox, dtype=np.int32)
    extent = np.array([X, Y, Z], np.float64) * VOXEL
    q = lo + rng.random((M, 3)) * extent
    n_far = M if variant == "all_empty" else (0 if variant == "one_sided" else int(round(EMPTY_SHARE * M)))
    far = rng.permutation(M)[:n_far]
    q[far] += 40.0
    new_xyz = q.astype(np.float32)
    cell = np.floor((new_xyz.astype(np.float64) - lo) / VOXEL).astype(np.int32)                  # (x, y, z)
    new_coords = np.concatenate([np.zeros((M, 1), np.int32), cell[:, ::-1]], 1)                 # [b, z, y, x]
    idx_raw = O.voxel_query(max_range, radius, nsample, xyz, new_xyz, np.ascontiguousarray(new_coords), v2p)
    if variant == "one_sided":
        new_xyz = new_xyz.copy()
        new_xyz[:, 0] -= np.float32(ONE_SIDED_SHIFT)
    return dict(M=M, nsample=nsample, C=C, eps=EPS, xyz=xyz, new_xyz=new_xyz, idx_raw=idx_raw,
                feats=rng.standard_normal((n_vox, C)).astype(np.float32),
                w_pos=(rng.standard_normal((C, 3)) * np.array([1.0, 0.7, 1.6])).astype(np.float32),
                gamma=rng.uniform(0.5, 1.5, C).astype(np.float32),
                beta=(rng.uniform(0.2, 0.6, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32),
                running_mean=rng.standard_normal(C).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C).astype(np.float32),
                cot=rng.standard_normal((C, M)).astype(np.float32))


def reference(case, train=True, stats_only=False, affine=True, requires_grad=False, dtype=None):
    """voxel_roi_pool_ref on a case -> (namespace, feats, w_pos, gamma, beta): the float64 leaves, for autograd.  affine
    False: no gamma / beta at all.  dtype: torch.float32 for the fp32 evaluation of the same chain."""
    import torch
    import torch_refs as R
    dtype = dtype or torch.float64
    t = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(requires_grad)   # noqa: E731
    feats, w = (None if stats_only else t(case["feats"])), t(case["w_pos"])
    gamma, beta = (t(case["gamma"]), t(case["beta"])) if affine else (None, None)
    ref = R.voxel_roi_pool_ref(torch.from_numpy(case["xyz"]), torch.from_numpy(case["new_xyz"]), feats,
                               torch.from_numpy(case["idx_raw"]), w, gamma, beta, case["eps"], train,
                               torch.from_numpy(case["running_mean"]), torch.from_numpy(case["running_var"]), dtype=dtype)
    return ref, feats, w, gamma, beta
