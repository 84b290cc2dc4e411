"""Plain-torch float64 reference implementations (autograd-capable) of the fused ops, used
by the GPU tests for value AND gradient parity.  They restate the published definitions
independently of both the HIP kernels and the C oracle."""
import math
from types import SimpleNamespace

import numpy as np
import torch


def roi_align_ref(inp, rois, out_size, scale, sampling_ratio=-1, aligned=False):
    """RoIAlign in float64 with autograd.  out_size: int or (ph, pw).  Every bin is summed on its own -- one gather of
    its bilinear taps from the (C, H*W) plane of its image, weights applied, taps added up -- and the bins are stacked at
    the end, so autograd never copies a (C, ph, pw) block per tap.  Same arithmetic per tap as the published definition;
    only the order in which one bin's taps are added differs from a running sum (reassociation, a few ulp of float64)."""
    inp = inp.double()
    K = rois.shape[0]
    N, C, H, W = inp.shape
    ph, pw = (out_size, out_size) if isinstance(out_size, int) else out_size
    planes = [inp[b].reshape(C, H * W) for b in range(N)]       # one select per image, shared by all of its RoIs
    off = 0.5 if aligned else 0.0
    zero = torch.zeros(C, dtype=torch.float64, device=inp.device)
    bins = []
    for k in range(K):
        b = int(rois[k, 0].item())
        x1, y1, x2, y2 = [float(v) * scale - off for v in rois[k, 1:]]
        rw, rh = x2 - x1, y2 - y1
        if not aligned:
            rw, rh = max(rw, 1.0), max(rh, 1.0)
        bw, bh = rw / pw, rh / ph
        gh = sampling_ratio if sampling_ratio > 0 else math.ceil(rh / ph)
        gw = sampling_ratio if sampling_ratio > 0 else math.ceil(rw / pw)
        count = max(gh * gw, 1)
        for p_h in range(ph):
            for p_w in range(pw):
                idx, wgt = [], []
                for iy in range(gh):
                    y = y1 + p_h * bh + (iy + 0.5) * bh / gh
                    for ix in range(gw):
                        x = x1 + p_w * bw + (ix + 0.5) * bw / gw
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yy, xx = max(y, 0.0), max(x, 0.0)
                        yl, xl = int(yy), int(xx)
                        if yl >= H - 1:
                            yh = yl = H - 1; yy = float(yl)
                        else:
                            yh = yl + 1
                        if xl >= W - 1:
                            xh = xl = W - 1; xx = float(xl)
                        else:
                            xh = xl + 1
                        ly, lx = yy - yl, xx - xl
                        hy, hx = 1 - ly, 1 - lx
                        idx += [yl * W + xl, yl * W + xh, yh * W + xl, yh * W + xh]
                        wgt += [hy * hx, hy * lx, ly * hx, ly * lx]
                if not idx:
                    bins.append(zero)
                    continue
                taps = planes[b][:, torch.tensor(idx, device=inp.device)] * torch.tensor(wgt, dtype=torch.float64, device=inp.device)
                bins.append(taps.sum(1) / count)
    return torch.stack(bins).reshape(K, ph, pw, C).permute(0, 3, 1, 2) if K else inp.new_zeros((0, C, ph, pw))


def dafm_ref(q, k, v, de, sigma, scale):
    e = torch.softmax(-(de / sigma), dim=1)
    att = torch.softmax((q @ k.T) * e * scale, dim=1)
    return att @ v, att


def gatv2_ref(x, edge_index, lin_l, lin_r, att, bias, heads, out_ch, slope=0.2, concat=False, edge_scale=None,
              add_self_loops=True, share_weights=False, return_alpha=False):
    """Dense-loop GATv2 as PyG's GATv2Conv computes it.  add_self_loops: input self loops are dropped and one loop per
    node is appended (otherwise the list is used as it is; a target without incoming edge then aggregates nothing and its
    row is the bias).  Duplicate edges stay duplicates: each takes part in the softmax.  share_weights: x_r = x_l = lin_l(x).
    bias may be None.  edge_scale: dict {(j, i): (H,) tensor} or None (it cannot tell duplicates apart: use it on graphs
    without them).  return_alpha: also the (E', H) attention in CSR order -- grouped by target, ascending; within a
    target in the order of the list (kept input edges first, the appended self loop last) -- before edge_scale."""
    n = x.shape[0]
    xl = lin_l(x).view(n, heads, out_ch)
    xr = xl if share_weights else lin_r(x).view(n, heads, out_ch)
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    if add_self_loops:
        pairs = [(j, i) for j, i in zip(src, dst) if j != i] + [(i, i) for i in range(n)]
    else:
        pairs = list(zip(src, dst))
    incoming = [[] for _ in range(n)]
    for j, i in pairs:
        incoming[i].append(j)
    out, alphas = [], []
    a = att.view(heads, out_ch)
    for i in range(n):
        js = incoming[i]
        z = torch.nn.functional.leaky_relu(xl[js] + xr[i][None], slope)      # (deg, H, C)
        e = (z * a[None]).sum(-1)                                           # (deg, H)
        al = torch.softmax(e, dim=0)
        alphas.append(al)
        if edge_scale is not None and js:
            al = al * torch.stack([edge_scale[(j, i)] for j in js])
        out.append((al[:, :, None] * xl[js]).sum(0))
    out = torch.stack(out)
    out = out.reshape(n, heads * out_ch) if concat else out.mean(1)
    if bias is not None:
        out = out + bias
    return (out, torch.cat(alphas)) if return_alpha else out


def voxel_roi_pool_ref(xyz, new_xyz, feats, idx_raw, w_pos, gamma, beta, eps, train, running_mean=None, running_var=None,
                       momentum=0.1, dtype=torch.float64):
    """One scale of the reference's NeighborVoxelSAModuleMSG between mlps_in and mlps_out (voxel_pool_modules.py:86-126)
    as its op chain, in float64 with autograd: gather the voxel rows, zero the rows of empty neighbourhoods
    (idx_raw[m, 0] == -1), relative coordinates r, p = w_pos . r, BatchNorm2d over ALL M * nsample columns (the biased
    variance normalises, the unbiased one goes into the running update; empty columns count), add the features, ReLU,
    max over nsample.  Every statistic is MEASURED on the (M, C, nsample) tensor; nothing here is a closed form.

    xyz (N, 3), new_xyz (M, 3), idx_raw (M, nsample) integer; feats (N, C) or None (statistics only: the returned
    pooled / pre / arg are None); w_pos (C, 3); gamma / beta (C) or None (no affine); train False normalises with
    running_mean / running_var.  Tensors that require grad must already be float64.  dtype=torch.float32 evaluates the
    same chain in fp32 (the yardstick for cancellation-limited sums, see test_voxel_roi_pool_gpu.py); everything that is
    compared against is the float64 default.

    Returns a namespace: pooled (C, M), pre (M, C, nsample) before the ReLU, arg (M, C) the FIRST slot that attains the
    maximum, mean / var (C; var biased), moments (10) = E[r], Cov(r) (biased: xx, xy, xz, yy, yz, zz), n, r (M, nsample,
    3), and running_mean / running_var after the momentum update (None where none was given).  n == 1 has no unbiased
    variance (torch refuses to train on one value per channel); the running update then keeps the biased one, 0."""
    f64 = lambda t: None if t is None else torch.as_tensor(t).to(dtype)   # noqa: E731
    xyz, new_xyz, w_pos, gamma, beta = f64(xyz), f64(new_xyz), f64(w_pos), f64(gamma), f64(beta)
    idx = torch.as_tensor(idx_raw).long()
    n_query, nsample = idx.shape
    empty = idx[:, 0] == -1
    rows = idx.clamp_min(0).masked_fill(empty[:, None], 0)
    keep = (~empty).to(dtype)
    r = (xyz[rows] - new_xyz[:, None, :]) * keep[:, None, None]                                  # (M, ns, 3)
    p = torch.einsum("ck,msk->mcs", w_pos, r)                                                    # (M, C, ns)
    n = n_query * nsample
    if train:
        mean = p.mean(dim=(0, 2))
        var = ((p - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    else:
        mean, var = f64(running_mean), f64(running_var)
    bn = (p - mean[None, :, None]) / torch.sqrt(var[None, :, None] + eps)
    if gamma is not None:
        bn = bn * gamma[None, :, None]
    if beta is not None:
        bn = bn + beta[None, :, None]
    out = SimpleNamespace(pooled=None, pre=None, arg=None, mean=mean, var=var, r=r, running_mean=None, running_var=None)
    flat = r.detach().reshape(-1, 3)
    er = flat.mean(0)
    cov = (flat - er).t() @ (flat - er) / max(n, 1)
    out.moments = torch.stack([er[0], er[1], er[2], cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2],
                               torch.tensor(float(n), dtype=dtype)])
    if train and running_mean is not None:
        out.running_mean = (1.0 - momentum) * f64(running_mean) + momentum * mean.detach()
    if train and running_var is not None:
        unbiased = var.detach() * (n / (n - 1.0)) if n > 1 else var.detach()
        out.running_var = (1.0 - momentum) * f64(running_var) + momentum * unbiased
    if feats is None:
        return out
    feats = torch.as_tensor(feats)
    g = feats[rows].permute(0, 2, 1) * keep[:, None, None]                                        # (M, C, ns)
    pre = g + bn
    top = pre.detach().max(dim=2, keepdim=True).values
    slots = torch.arange(nsample).expand_as(pre)
    arg = torch.where(pre.detach() == top, slots, torch.full_like(slots, nsample)).min(dim=2).values
    # max over nsample through the first arg-max slot: equal values (first-hit padding repeats a row) carry equal gradients
    out.pooled = torch.relu(pre.gather(2, arg[:, :, None]).squeeze(2)).t()
    out.pre, out.arg = pre, arg
    return out


def near_tie_mask(values, idx_raw, margin):
    """(M, C) bool: entries whose best value over nsample is closer than margin * max |values| to the best value of a
    DIFFERENT voxel row -- there an fp32 evaluation may legitimately pick another neighbour than float64 does.  values
    (M, C, nsample), idx_raw (M, nsample).  A row repeated by first-hit padding carries an identical value in every
    evaluation and is no tie: both sides take the first slot.  Empty neighbourhoods are one (zero) row: never masked."""
    values = values.detach()
    idx = torch.as_tensor(idx_raw).long()
    if values.numel() == 0:
        return torch.zeros(values.shape[:2], dtype=torch.bool)
    empty = idx[:, 0] == -1
    rows = idx.clamp_min(0).masked_fill(empty[:, None], 0)
    best, slot = values.max(dim=2)
    best_row = rows.gather(1, slot)                                                               # (M, C)
    other = rows[:, None, :] != best_row[:, :, None]                                              # (M, C, ns)
    rival = values.masked_fill(~other, -math.inf).max(dim=2).values
    return (best - rival) < margin * values.abs().max()


# ---------------------------------------------------------------------------------------------- query and group
# Float64 references of csrc/query_group.hip, and the rounding-count bounds its device test asserts
# (tests/test_query_group_gpu.py; tests/test_query_group_cpu.py proves them satisfiable).  U32 = fp32 unit roundoff.
U32 = 2.0 ** -24
TINY32 = 2.0 ** -149


def query_group_batch_ref(xyz, new_xyz, feats_or_zf, idx, wx=None):
    """QueryAndGroup after the ball query, dense batches, in float64 from the fp32 operands.  xyz (b, n, 3), new_xyz
    (b, m, 3), feats_or_zf (b, c, n) or None (c = 0), idx (b, m, ns) -> rel (b, 3, m, ns), y (b, c, m, ns) = the gathered
    rows, plus wx (c, 3) . rel when wx is given ("project, then group").  Autograd flows through feats_or_zf and wx
    (hand them in as float64 leaves)."""
    xyz, new_xyz = torch.as_tensor(xyz).double(), torch.as_tensor(new_xyz).double()
    idx = torch.as_tensor(idx).long()
    b, m, ns = idx.shape
    flat = idx.reshape(b, m * ns)
    near = torch.gather(xyz, 1, flat[:, :, None].expand(-1, -1, 3)).view(b, m, ns, 3)
    rel = (near - new_xyz[:, :, None, :]).permute(0, 3, 1, 2)
    if feats_or_zf is None:
        y = rel.new_zeros((b, 0, m, ns))
    else:
        f = torch.as_tensor(feats_or_zf).double()
        y = torch.gather(f, 2, flat[:, None, :].expand(-1, f.shape[1], -1)).view(b, f.shape[1], m, ns)
    if wx is not None:
        y = y + torch.einsum("ck,bkms->bcms", torch.as_tensor(wx).double(), rel)
    return rel, y


def stack_source_rows(xyz_cnt, new_cnt, idx_raw):
    """(M, ns) int64: the global source row of every column of the raw stacked ball-query result, -1 for every slot of
    an empty ball (idx_raw[row][0] == -1; its other slots hold arbitrary values and are ignored)."""
    xyz_cnt, new_cnt = np.asarray(xyz_cnt, np.int64), np.asarray(new_cnt, np.int64)
    idx = np.asarray(idx_raw, np.int64)
    start = np.concatenate([[0], np.cumsum(xyz_cnt)[:-1]])
    rows = idx + np.repeat(start, new_cnt)[:, None]
    rows[idx[:, 0] == -1] = -1
    return rows


def query_group_stack_ref(xyz, xyz_cnt, new_xyz, new_cnt, feats_or_zf, idx_raw, wx=None):
    """The same for stacked batches in the channel-major layout: xyz (N, 3), new_xyz (M, 3), feats_or_zf (N, C) (any
    row stride) or None, idx_raw (M, ns) sample-local with the raw ball-query convention -> rel (3, M * ns), y
    (C, M * ns).  The columns of an empty ball are zero in rel and y and carry nothing backward."""
    xyz, new_xyz = torch.as_tensor(xyz).double(), torch.as_tensor(new_xyz).double()
    rows = torch.from_numpy(stack_source_rows(xyz_cnt, new_cnt, idx_raw))
    m, ns = rows.shape
    live = rows[:, 0] >= 0
    keep = live.double()[:, None, None]
    src = torch.where(live[:, None], rows, torch.zeros_like(rows))
    zeros3 = xyz.new_zeros((m, ns, 3))
    rel = ((xyz[src] if xyz.shape[0] else zeros3) - new_xyz[:, None, :]) * keep
    rel = rel.permute(2, 0, 1).reshape(3, m * ns)
    if feats_or_zf is None:
        y = rel.new_zeros((0, m * ns))
    else:
        f = torch.as_tensor(feats_or_zf).double()
        g = f[src] if f.shape[0] else f.new_zeros((m, ns, f.shape[1]))
        y = (g * keep).permute(2, 0, 1).reshape(f.shape[1], m * ns)
    if wx is not None:
        y = y + torch.as_tensor(wx).double() @ rel
    return rel, y


def qg_tile_stats_ref(y, chunk=128):
    """y (C, T) with T % chunk == 0 -> float64 (tile_mean (C, T / chunk), tile_m2 (C, T / chunk), mean (C), var (C)):
    per channel and tile of `chunk` consecutive columns the mean and the sum of squared deviations from it, and the
    BatchNorm mean / biased variance the tiles finalise to through Chan's merge
    (M2 = sum_t M2_t + chunk * sum_t (mean_t - mean)^2)."""
    y = torch.as_tensor(y).detach().double()
    c, t = y.shape
    assert t % chunk == 0
    tiles = y.view(c, t // chunk, chunk)
    tile_mean = tiles.mean(2)
    tile_m2 = ((tiles - tile_mean[:, :, None]) ** 2).sum(2)
    mean = tile_mean.mean(1)
    var = (tile_m2.sum(1) + chunk * ((tile_mean - mean[:, None]) ** 2).sum(1)) / max(t, 1)
    return tile_mean, tile_m2, mean, var


def qg_scatter_batch_ref(g, idx, n):
    """Backward of the batch gather: g (b, c, cols), idx (b, cols) -> float64 numpy (want (b, c, n), k (b, 1, n) the
    number of contributions of every cell, sabs (b, c, n) = sum |g| over them), by np.add.at."""
    g, idx = np.asarray(g, np.float64), np.asarray(idx, np.int64)
    b, c, _ = g.shape
    want, sabs = np.zeros((b, c, n)), np.zeros((b, c, n))
    for bi in range(b):
        for ci in range(c):
            np.add.at(want[bi, ci], idx[bi], g[bi, ci])
            np.add.at(sabs[bi, ci], idx[bi], np.abs(g[bi, ci]))
    k = np.stack([np.bincount(idx[bi], minlength=n) for bi in range(b)])[:, None, :].astype(np.float64)
    return want, k, sabs


def qg_scatter_stack_ref(g, rows, n):
    """Backward of the stack gather: g (C, M * ns), rows = stack_source_rows(...) -> float64 numpy (want (n, C),
    k (n, 1), sabs (n, C)); the columns of empty balls (row -1) contribute nothing."""
    g, rows = np.asarray(g, np.float64), np.asarray(rows, np.int64).reshape(-1)
    live = rows >= 0
    want, sabs = np.zeros((n, g.shape[0])), np.zeros((n, g.shape[0]))
    np.add.at(want, rows[live], g[:, live].T)
    np.add.at(sabs, rows[live], np.abs(g[:, live].T))
    k = np.bincount(rows[live], minlength=n)[:, None].astype(np.float64)
    return want, k, sabs


def qg_proj_fwd_bound(gathered, wx, rel):
    """Elementwise bound of the fp32 "project, then group" forward against float64: 6 u (|zf| + sum_i |wx_i| |rel_i|)
    + 2^-149.  One rounding in rel, one per product, two additions inside wx . rel and one onto zf: at most five on
    any term, (1 + u)^5 - 1 < 6 u.  Contracting a product and an addition into an FMA only removes roundings.
    gathered: |zf| at the columns, (b, c, m, ns) / (C, T); rel (b, 3, m, ns) / (3, T); wx (c, 3)."""
    gathered, rel, wx = (torch.as_tensor(t).detach().double().abs() for t in (gathered, rel, wx))
    mix = torch.einsum("ck,bkms->bcms", wx, rel) if rel.dim() == 4 else wx @ rel
    return 6.0 * U32 * (gathered + mix) + TINY32


def qg_fixed_point_scatter_bound(want, k, row_max, cols):
    """Bound of qg_batch_bwd_lds_kernel (order-free 64-bit fixed point): every cell is the float64 scatter-add within one
    fp32 rounding, plus k contributions each rounded by at most max|g of the row| * cols * 2^-61, plus the float64
    reference's own k * max|g| * 2^-50.  numpy arrays that broadcast to want."""
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + k * row_max * cols * 2.0 ** -61 \
        + k * row_max * 2.0 ** -50


def qg_atomic_scatter_bound(want, k, sabs):
    """Bound of a float-atomic scatter in any order: the first contribution lands exactly on the zeroed cell and each of
    the other k - 1 additions rounds a partial sum no larger than sum |g|: (k - 1) u sum|g| + spacing(fp32(want)).
    Cells nobody references (k = 0) get 0 here on purpose: they are asserted to be exactly 0."""
    return np.where(k > 0, np.maximum(k - 1.0, 0.0) * U32 * sabs + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 0.0)


def qg_tile_stats_bounds(y, chunk=128):
    """Bounds of the (mean, M2) partials qg_stack_fwd_kernel leaves per channel and 128-column tile, against
    qg_tile_stats_ref of the SAME fp32 y, from the kernel's summation shape:
      mean: eight sequential 16-term sums (15 roundings), a sequential sum of the eight (7 more), times 2^-7 (exact):
            |d mean| <= g(22) * mean|v|,  g(j) = j u / (1 - j u);
      M2:   two-pass about the computed mean: v - mean (1 rounding, squared: 2), the product (1), the same 15 + 7
            additions: sum (v - mean_hat)^2 (1 + t), |t| <= g(25), and sum (v - mean_hat)^2 = M2 + chunk * d mean^2:
            |d M2| <= g(25) * M2 + (1 + g(25)) * chunk * (d mean bound)^2.
    An all-zero tile gives (0, 0) exactly; 2^-149 covers an underflow of the scaling by 2^-7.
    Returns float64 (mean_bound, m2_bound), both (C, T / chunk)."""
    y = torch.as_tensor(y).detach().double()
    c, t = y.shape
    tiles = y.view(c, t // chunk, chunk)
    gamma = lambda j: j * U32 / (1.0 - j * U32)   # noqa: E731
    _, m2, _, _ = qg_tile_stats_ref(y, chunk)
    zero = (tiles == 0).all(2)
    dmean = gamma(22) * tiles.abs().mean(2) + TINY32
    dm2 = gamma(25) * m2 + (1.0 + gamma(25)) * chunk * dmean ** 2
    return dmean.masked_fill(zero, 0.0), dm2.masked_fill(zero, 0.0)


def qg_final_stats_bounds(y, eps, chunk=128):
    """Bounds of mean / invstd that mgar_bn_stats_from_partials finalises from those partials (Chan's merge in double, one
    fp32 rounding each at the end) against float64 of the same y.  With d = the largest tile-mean bound of the channel:
      |d mean| <= average tile-mean bound + u |mean|;
      |d var|  <= average(M2 bound) / chunk + average(4 d |mean_t - mean| + 4 d^2)     (both means move by <= d);
      |d invstd| <= |d var| / 2 * (var + eps - |d var|)^-3/2 + u * invstd              ((v + eps)^-1/2 is convex).
    Returns float64 (mean_bound (C), invstd_bound (C))."""
    tile_mean, _, mean, var = qg_tile_stats_ref(y, chunk)
    dmean_t, dm2_t = qg_tile_stats_bounds(y, chunk)
    d = dmean_t.max(1).values
    dvar = dm2_t.mean(1) / chunk + (4.0 * d[:, None] * (tile_mean - mean[:, None]).abs() + 4.0 * d[:, None] ** 2).mean(1)
    low = var + eps - dvar
    assert (low > 0).all()
    invstd = (var + eps) ** -0.5
    return dmean_t.mean(1) + U32 * mean.abs() + TINY32, 0.5 * dvar * low ** -1.5 + U32 * invstd


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm(train) + ReLU + max over nsample (csrc/bn_act.hip): float64 references in numpy and the rounding-count bounds of
# DESIGN.md section 5c.  gamma_u(j) = j u / (1 - j u) bounds (1 + u)^j - 1.
def gamma_u(j):
    return j * U32 / (1.0 - j * U32)


def bn_chunk(B, C, P):
    """Elements per workgroup of the statistics / backward reductions: bn_chunk() of bn_act.hip restated."""
    n, chunk = B * P, 65536
    while chunk > 4096 and -(-n // chunk) * C < 2048:
        chunk >>= 1
    return chunk


def bn_channel_major(x):
    """(B, C, P) -> float64 (C, B * P): the element order of a channel."""
    x = np.asarray(x, np.float64)
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(x.shape[1], -1)


def bn_stats_ref(x):
    """x (B, C, P) -> float64 (mean (C), biased variance (C))."""
    xc = bn_channel_major(x)
    mean = xc.mean(1)
    return mean, ((xc - mean[:, None]) ** 2).mean(1)


def bn_running_ref(means, variances, n, momentum, running_mean, running_var, dmean=None, dvar=None, roundings=6):
    """The momentum updates of rows g = 0.. of means / biased variances (G, C) in order, unbiased correction n / (n - 1) for
    n > 1, with the fp32 values of momentum and 1 - momentum the kernels use -> float64 (running_mean, running_var, bound,
    bound).  A step rounds each of its two terms at most `roundings` times (scaling, the unbiased factor in fp32 in the
    one-launch kernel, the addition) and carries the statistics' own bounds dmean / dvar (G, C) scaled by momentum."""
    means, variances = np.atleast_2d(np.asarray(means, np.float64)), np.atleast_2d(np.asarray(variances, np.float64))
    mom, om = float(np.float32(momentum)), float(np.float32(1.0) - np.float32(momentum))
    k = n / (n - 1.0) if n > 1 else 1.0
    rm, rv = np.asarray(running_mean, np.float64).copy(), np.asarray(running_var, np.float64).copy()
    brm, brv = np.zeros_like(rm), np.zeros_like(rv)
    zero = np.zeros_like(means)
    dmean, dvar = (zero if dmean is None else np.atleast_2d(dmean)), (zero if dvar is None else np.atleast_2d(dvar))
    for g in range(means.shape[0]):
        brm = om * brm + mom * dmean[g] + roundings * U32 * (np.abs(om * rm) + np.abs(mom * means[g])) + TINY32
        brv = om * brv + mom * k * dvar[g] + roundings * U32 * (np.abs(om * rv) + np.abs(mom * k * variances[g])) + TINY32
        rm = om * rm + mom * means[g]
        rv = om * rv + mom * k * variances[g]
    return rm, rv, brm, brv


def _per_channel(a, B, C, per_sample):
    return np.asarray(a, np.float64).reshape((B, C, 1) if per_sample else (1, C, 1))


def bn_apply_ref(x, mean, invstd, gamma, beta, relu, per_sample=False):
    """y = [relu]((x - mean) * invstd * gamma + beta) in float64 of the given (fp32) mean / invstd (C, or B * C with
    per-sample statistics) -> (pre-activation, y, bound).  bound = 4 u (|x - mean| |sc| + |pre|) + 2^-149: x - mean,
    sc = invstd * gamma, the product (three roundings on the first term), the addition (one on the sum); a ReLU is
    1-Lipschitz and adds nothing."""
    x = np.asarray(x, np.float64)
    B, C, _ = x.shape
    mu, inv = _per_channel(mean, B, C, per_sample), _per_channel(invstd, B, C, per_sample)
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    sc = inv * g.reshape(1, C, 1)
    pre = (x - mu) * sc + b.reshape(1, C, 1)
    bound = 4.0 * U32 * (np.abs(x - mu) * np.abs(sc) + np.abs(pre)) + TINY32
    return pre, (np.maximum(pre, 0.0) if relu else pre), bound


def bn_max_ref(pre, relu):
    """pre (B, C, M, ns) float64 -> (max over ns [after ReLU], FIRST arg-max of the pre-ReLU values)."""
    arg = np.argmax(pre, axis=-1)                     # numpy: the first occurrence
    best = np.take_along_axis(pre, arg[..., None], -1)[..., 0]
    return (np.maximum(best, 0.0) if relu else best), arg


def bn_bwd_ref(dz, x, mean, invstd, gamma, n=None):
    """Closed-form backward of y = bn_train(x) * gamma + beta given dz = the gradient behind the ReLU mask, all (B, C, P),
    in float64 of the given mean / invstd: dbeta = sum dz, dgamma = sum dz xh, coef = (dbeta, dgamma) / n,
    dx = invstd gamma (dz - coef0 - xh coef1).  -> dict with those and the absolute sums the bounds need."""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    B, C, P = x.shape
    n = B * P if n is None else n
    mu, inv = _per_channel(mean, B, C, False), _per_channel(invstd, B, C, False)
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    xh = (x - mu) * inv
    dbeta, dgamma = dz.sum((0, 2)), (dz * xh).sum((0, 2))
    coef = np.stack([dbeta, dgamma], 1) / n
    k = inv * g.reshape(1, C, 1)
    dx = k * (dz - coef[:, 0].reshape(1, C, 1) - xh * coef[:, 1].reshape(1, C, 1))
    return dict(dbeta=dbeta, dgamma=dgamma, coef=coef, dx=dx, xh=xh, k=k, dz=dz, n=n,
                sabs_beta=np.abs(dz).sum((0, 2)), sabs_gamma=np.abs(dz * xh).sum((0, 2)))


def bn_bwd_bounds(r, longest_lane_chain, coef_given=False):
    """Bounds of dbeta, dgamma, coef and dx for a bn_bwd_ref result.  longest_lane_chain = additions a lane makes before the
    64-lane tree (6) and the 4-wave sum (3): a term of dbeta passes depth = chain + 9 roundings, a term of dgamma three
    more (x - mean, * invstd, * dz); the chunks are summed in double and rounded once.  dx = k (d - m0 - xh m1): k, x - mean,
    * invstd, * m1, d - m0, the difference, * k: at most 7 roundings on a term, plus the bounds of m0, m1 scaled by |k|,
    |k xh| (0 when the caller supplies coef)."""
    depth = longest_lane_chain + 9
    bbeta = gamma_u(depth) * r["sabs_beta"] + U32 * np.abs(r["dbeta"]) + TINY32
    bgamma = gamma_u(depth + 3) * r["sabs_gamma"] + U32 * np.abs(r["dgamma"]) + TINY32
    bcoef = np.stack([bbeta, bgamma], 1) / r["n"] + U32 * np.abs(r["coef"]) + TINY32
    if coef_given:
        bcoef = np.zeros_like(bcoef)
    C = r["coef"].shape[0]
    m0, m1 = r["coef"][:, 0].reshape(1, C, 1), r["coef"][:, 1].reshape(1, C, 1)
    ak = np.abs(r["k"])
    bdx = gamma_u(7) * ak * (np.abs(r["dz"]) + np.abs(m0) + np.abs(r["xh"] * m1)) \
        + (1.0 + gamma_u(7)) * ak * (bcoef[:, 0].reshape(1, C, 1) + np.abs(r["xh"]) * bcoef[:, 1].reshape(1, C, 1)) + TINY32
    return bbeta, bgamma, bcoef, bdx


def bn_chan_merge_ref(cnt, mean_k, m2_k):
    """Chan et al.: chunks of cnt (K) elements with means / sums of squared deviations (C, K) -> float64 (mean, M2) (C)."""
    cnt, mean_k, m2_k = (np.asarray(a, np.float64) for a in (cnt, mean_k, m2_k))
    mean = (cnt * mean_k).sum(1) / cnt.sum()
    return mean, m2_k.sum(1) + (cnt * (mean_k - mean[:, None]) ** 2).sum(1)


def bn_partial_stats_bounds(xc, chunk, vec):
    """What bn_partial_kernel leaves per (channel, chunk) of xc (C, n) float64, and how far off it may be:
    (cnt (K), mean_k, M2_k, dmean_k, dM2_k (C, K)).  Per chunk of nk elements, with p the mean of its first min(256, nk)
    elements (the pivot; the kernel's fp32 p_hat is within dp = gamma_u(10) mean|first elements| of it: 6 + 3 additions, the
    division) and L = ceil(nk / 256 [/ 4 with float4 loads]) additions per lane:
      s = sum (x - p_hat): x - p_hat (1 rounding), the float4's pair tree (2), L, the 64-lane tree (6), 4 waves (3):
          |ds| <= gamma_u(L + 12) * A1,  A1 = sum (|x - p| + dp);
      chunk mean = p_hat + s / nk in double, rounded once:  dmean = |ds| / nk + u |mean_k|;
      q = sum (x - p_hat)^2: two more roundings per term: |dq| <= gamma_u(L + 14) * A2,  A2 = sum (|x - p| + dp)^2;
      M2 = q - s^2 / nk in double, rounded once:  dM2 = |dq| + (2 |s| |ds| + ds^2) / nk + u M2,  |s| <= nk (|mean_k - p| + dp).
    Nothing here grows with |mean| but u |mean_k| (and dp, which enters squared or times u)."""
    C, n = xc.shape
    out = []
    for e0 in range(0, n, chunk):
        v = xc[:, e0:e0 + chunk]
        nk = v.shape[1]
        npiv = min(256, nk)
        p = v[:, :npiv].mean(1, keepdims=True)
        dp = gamma_u(10) * np.abs(v[:, :npiv]).mean(1, keepdims=True)
        L = -(-nk // (256 * (4 if vec else 1)))
        dev_ = np.abs(v - p) + dp
        a1, a2 = dev_.sum(1), (dev_ ** 2).sum(1)
        mean_k = v.mean(1)
        m2_k = ((v - mean_k[:, None]) ** 2).sum(1)
        ds = gamma_u(L + 12) * a1
        s_abs = nk * (np.abs(mean_k - p[:, 0]) + dp[:, 0])
        dmean = ds / nk + U32 * np.abs(mean_k) + TINY32
        dm2 = gamma_u(L + 14) * a2 + (2.0 * s_abs * ds + ds * ds) / nk + U32 * m2_k + TINY32
        out.append((float(nk), mean_k, m2_k, dmean, dm2))
    cnt = np.array([o[0] for o in out])
    return (cnt,) + tuple(np.stack([o[i] for o in out], 1) for i in (1, 2, 3, 4))


def bn_merge_bounds(cnt, mean_k, m2_k, dmean_k, dm2_k, eps):
    """bn_finalize_kernel: Chan's merge in double of partials that are within dmean_k / dM2_k of the true ones, one fp32
    rounding each of mean and invstd -> float64 (mean, var, mean bound, invstd bound, var bound), as qg_final_stats_bounds:
      |d mean| <= sum n_k dmean_k / n + u |mean|;
      |d var|  <= [sum dM2_k + sum n_k (4 d |mean_k - mean| + 4 d^2)] / n,  d = max_k dmean_k (both means move by <= d);
      |d invstd| <= |d var| / 2 (var + eps - |d var|)^-3/2 + u invstd."""
    cnt = np.asarray(cnt, np.float64)
    n = cnt.sum()
    mean, m2 = bn_chan_merge_ref(cnt, mean_k, m2_k)
    var = m2 / n
    d = dmean_k.max(1)[:, None]
    dvar = (dm2_k.sum(1) + (cnt * (4.0 * d * np.abs(mean_k - mean[:, None]) + 4.0 * d * d)).sum(1)) / n
    low = var + eps - dvar
    assert (low > 0).all()
    invstd = (var + eps) ** -0.5
    return mean, var, (cnt * dmean_k).sum(1) / n + U32 * np.abs(mean) + TINY32, 0.5 * dvar * low ** -1.5 + U32 * invstd, dvar


def bn_train_stats_bounds(x, eps):
    """mgar_bn_train_stats on x (B, C, P): float64 (mean, var, mean bound, invstd bound, var bound)."""
    B, C, P = x.shape
    parts = bn_partial_stats_bounds(bn_channel_major(x), bn_chunk(B, C, P), P % 4 == 0)
    return bn_merge_bounds(*parts, eps)


def bn_from_partials_bounds(cnt, mean_k, m2_k, eps, group=256, direct_max=1024):
    """mgar_bn_stats_from_partials on fp32 partials (C, K): up to 1 024 chunks are merged in double in one step; more are
    first merged in groups of 256, whose (mean, M2) are rounded to fp32 (u |mean_g|, u M2_g) before the same final merge.
    2^-40 relative covers the double arithmetic."""
    cnt, mean_k, m2_k = (np.asarray(a, np.float64) for a in (cnt, mean_k, m2_k))
    dd = 2.0 ** -40
    if len(cnt) > direct_max:
        gc, gm, gq = [], [], []
        for i in range(0, len(cnt), group):
            m, q = bn_chan_merge_ref(cnt[i:i + group], mean_k[:, i:i + group], m2_k[:, i:i + group])
            gc.append(cnt[i:i + group].sum()), gm.append(m), gq.append(q)
        cnt, mean_k, m2_k = np.array(gc), np.stack(gm, 1), np.stack(gq, 1)
        dd += U32
    return bn_merge_bounds(cnt, mean_k, m2_k, dd * np.abs(mean_k) + TINY32, dd * m2_k + TINY32, eps)


# ---------------------------------------------------------------------------------------------------------------------
# Channels-last / row-major BatchNorm (csrc/channels_last.hpp) and 3-D max pooling (csrc/maxpool3d.hip).
CL_THREADS = 256


def bn_cl_chunk_rows(S, R):
    """Rows per statistics chunk: cl_chunk_rows() of channels_last.hpp restated (at least 256 rows, about 2 048 workgroups
    in all, never more than R).  Statistics over all samples call it as (1, S * R)."""
    return int(min(max(-(-(S * R) // 2048), 256), R))


def bn_cl_partial_stats_bounds(xr, chunk):
    """What bn_cl_partial_kernel leaves per (channel, chunk) of the rows xr (R, C) float64 of one statistics group, and how far
    off it may be: (cnt (K), mean_k, M2_k, dmean_k, dM2_k (C, K)), the format of bn_partial_stats_bounds.  Per chunk of nk rows,
    with p = the chunk's FIRST row (the pivot, an input value: exact, dp = 0), rpar = 256 // (C / 4) row lanes, L = ceil(nk /
    rpar) additions per lane and rpar - 1 more when the lanes are added in order:
      s = sum (x - p): x - p (1 rounding) and at most L + rpar - 1 additions:  |ds| <= gamma_u(L + rpar) * A1,  A1 = sum |x - p|;
      q = sum (x - p)^2: two more roundings per term:                          |dq| <= gamma_u(L + rpar + 2) * A2,  A2 = sum (x - p)^2;
      chunk mean = p + s / nk in double, rounded once:  dmean = |ds| / nk + u |mean_k|;
      M2 = q - s^2 / nk in double, rounded once:  dM2 = |dq| + (2 |s| |ds| + ds^2) / nk + u M2,  |s| = nk |mean_k - p|."""
    xr = np.asarray(xr, np.float64)
    rows, C = xr.shape
    rpar = CL_THREADS // (C // 4)
    out = []
    for r0 in range(0, rows, chunk):
        v = xr[r0:r0 + chunk]
        nk = v.shape[0]
        p = v[0]
        L = -(-nk // rpar)
        dev_ = np.abs(v - p)
        a1, a2 = dev_.sum(0), (dev_ ** 2).sum(0)
        mean_k = v.mean(0)
        m2_k = ((v - mean_k) ** 2).sum(0)
        ds = gamma_u(L + rpar) * a1
        s_abs = nk * np.abs(mean_k - p)
        dmean = ds / nk + U32 * np.abs(mean_k) + TINY32
        dm2 = gamma_u(L + rpar + 2) * a2 + (2.0 * s_abs * ds + ds * ds) / nk + U32 * m2_k + TINY32
        out.append((float(nk), mean_k, m2_k, dmean, dm2))
    cnt = np.array([o[0] for o in out])
    return (cnt,) + tuple(np.stack([o[i] for o in out], 1) for i in (1, 2, 3, 4))


def bn_cl_train_stats_bounds(x, per_sample, eps):
    """mgar_bn_cl_train_stats on x (S, R, C): float64 (mean, var, mean bound, invstd bound, var bound), each (C), or (S * C)
    with per-sample statistics (sample-major, as the entry point writes them)."""
    x = np.asarray(x, np.float64)
    S, Rr, C = x.shape
    if per_sample:
        chunk = bn_cl_chunk_rows(S, Rr)
        parts = [bn_merge_bounds(*bn_cl_partial_stats_bounds(x[s], chunk), eps) for s in range(S)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))
    return bn_merge_bounds(*bn_cl_partial_stats_bounds(x.reshape(S * Rr, C), bn_cl_chunk_rows(1, S * Rr)), eps)


def bn_rows_bwd_lane_chain(rows, C):
    """The longest chain of additions of bn_rows_bwd_partial_kernel: a row lane's ceil(chunk / rpar), then the rpar lanes in
    order (the argument of bn_bwd_bounds)."""
    rpar = CL_THREADS // (C // 4)
    return -(-bn_cl_chunk_rows(1, rows) // rpar) + rpar - 1


def same_pads(size, k, s):
    """(front, back) zero padding of one axis of the reference's MaxPool3dSamePadding (model/backbone.py compute_pad)."""
    total = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return total // 2, total - total // 2


def maxpool3d_ref(x, k, s, pad_value):
    """x (..., T, H, W) -> (..., ceil(T / st), ceil(H / sh), ceil(W / sw)) float64: pad every axis by same_pads with
    pad_value (0: the zero padding takes part, "same"; -inf: only the input's own elements count, "valid"), then the maximum
    of every k window at stride s.  A NaN in a window is its maximum (np.max, as torch.max_pool3d).  Exact: no bound."""
    x = np.asarray(x, np.float64)
    pads = [same_pads(x.shape[-3 + i], k[i], s[i]) for i in range(3)]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 3) + pads, constant_values=pad_value)
    win = np.lib.stride_tricks.sliding_window_view(xp, tuple(k), axis=(-3, -2, -1))
    return win[..., ::s[0], ::s[1], ::s[2], :, :, :].max(axis=(-3, -2, -1))
