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
