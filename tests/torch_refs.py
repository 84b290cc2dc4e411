"""Plain-torch float64 reference implementations (autograd-capable) of the fused ops, used
by the GPU tests for value AND gradient parity.  They restate the published definitions
independently of both the HIP kernels and the C oracle."""
import math
from types import SimpleNamespace

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
