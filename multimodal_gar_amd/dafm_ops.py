"""Fused DAFM attention core (HIP): E = softmax(-De/sigma), Att = softmax(QK^T * E * scale),
out = Att V -- model/gat_model.py:487-491, :503-505 -- batched over scenes."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L


class _DafmAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, de_flat, scene_off, de_off, sigma, scale):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        rows, d = q.shape
        n_scenes = scene_off.numel() - 1
        att = torch.empty_like(de_flat)
        out = torch.empty_like(q)
        L.call("mgar_dafm_attn_fwd", n_scenes, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(q), L.fptr(k),
               L.fptr(v), L.fptr(de_flat), float(sigma), float(scale), L.fptr(att), L.fptr(out), L.stream_of(q))
        ctx.save_for_backward(q, k, v, de_flat, scene_off, de_off, att)
        ctx.cfg = (float(sigma), float(scale))
        ctx.mark_non_differentiable(att)      # backward has no gradient path through att
        return out, att

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_att_unused):
        q, k, v, de_flat, scene_off, de_off, att = ctx.saved_tensors
        sigma, scale = ctx.cfg
        rows, d = q.shape
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        gmat = torch.empty_like(att)
        grad_out = grad_out.contiguous()
        L.call("mgar_dafm_attn_bwd", scene_off.numel() - 1, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(q),
               L.fptr(k), L.fptr(v), L.fptr(de_flat), sigma, scale, L.fptr(att), L.fptr(grad_out),
               L.fptr(gmat), L.fptr(gq), L.fptr(gk), L.fptr(gv), L.stream_of(q))
        return gq, gk, gv, None, None, None, None, None


class _DafmAttentionAdd(Function):
    """Att = softmax(QK^T * scale + P), out = Att V; P is a constant of the graph (None gradient), or None."""

    @staticmethod
    def forward(ctx, q, k, v, prior_flat, scene_off, de_off, pairs, scale):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        rows, d = q.shape
        n_scenes = scene_off.numel() - 1
        att = torch.empty(pairs, dtype=q.dtype, device=q.device)
        out = torch.empty_like(q)
        L.call("mgar_dafm_attn_add_fwd", n_scenes, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(q), L.fptr(k),
               L.fptr(v), None if prior_flat is None else L.fptr(prior_flat), float(scale), L.fptr(att), L.fptr(out),
               L.stream_of(q))
        ctx.save_for_backward(q, k, v, scene_off, de_off, att)
        ctx.scale = float(scale)
        ctx.mark_non_differentiable(att)      # backward has no gradient path through att
        return out, att

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_att_unused):
        q, k, v, scene_off, de_off, att = ctx.saved_tensors
        rows, d = q.shape
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        gmat = torch.empty_like(att)
        grad_out = grad_out.contiguous()
        L.call("mgar_dafm_attn_add_bwd", scene_off.numel() - 1, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(q),
               L.fptr(k), L.fptr(v), ctx.scale, L.fptr(att), L.fptr(grad_out), L.fptr(gmat), L.fptr(gq), L.fptr(gk),
               L.fptr(gv), L.stream_of(q))
        return gq, gk, gv, None, None, None, None, None


_OFFSET_CACHE = {}


def packed_pairs(scene_off):
    """sum_s n_s^2, the floats of a packed (n_s, n_s)-per-scene tensor, READ FROM THE DEVICE: for callers that hold only
    the offsets.  A caller that knows its counts (scene_layout().pairs) passes the number instead and reads nothing."""
    so = scene_off.tolist()
    return sum((b - a) ** 2 for a, b in zip(so[:-1], so[1:]))


def scene_offsets(counts, device):
    """counts: python list of actors per scene -> (scene_off (S+1,), de_off (S,)) int32 on device.
    Cached per (counts, device): no host->device copy in the steady state (and none under graph capture).
    The kernels hold a scene's columns in registers, MGAR_DAFM_MAX_N (include/mgar_ops.h) at the most; the C entry sees
    only device pointers, so the limit is enforced here, where the counts are still a host list."""
    key = (tuple(int(c) for c in counts), str(device))
    hit = _OFFSET_CACHE.get(key)
    if hit is not None:
        return hit
    for n in counts:
        if not 0 <= int(n) <= L.DAFM_MAX_N:
            raise ValueError("dafm: a scene of %d actors is outside 0..%d (MGAR_DAFM_MAX_N), the capacity of the "
                             "attention kernels" % (int(n), L.DAFM_MAX_N))
    so, do, r, m = [0], [], 0, 0
    for n in counts:
        do.append(m)
        r += n
        m += n * n
        so.append(r)
    out = (torch.tensor(so, dtype=torch.int32, device=device), torch.tensor(do, dtype=torch.int32, device=device))
    if len(_OFFSET_CACHE) < 64:
        _OFFSET_CACHE[key] = out
    return out


def dafm_attention(q, k, v, de_flat, scene_off, de_off, sigma, scale):
    """q, k, v: (rows, D) stacked over scenes; de_flat: concatenation of each scene's (n, n)
    distance matrix, row-major.  Returns (out (rows, D), att (same layout as de_flat))."""
    # The per-scene attention tensors are tiny (A x 512 per scene): they stay fp32 on every configuration; under the bf16
    # configurations (autocast) the projections that produce q / k / v run as bf16 GEMMs and are widened here.
    return _DafmAttention.apply(q.float(), k.float(), v.float(), de_flat.float(), scene_off, de_off, sigma, scale)


def dafm_attention_add(q, k, v, prior_flat, scene_off, de_off, scale, pairs=None):
    """The attention core with an additive prior: Att = softmax(q k^T * scale + P, dim=1) per scene, out = Att v.
    prior_flat: each scene's (n, n) prior, flattened and concatenated like de_flat of dafm_attention, or None for plain
    attention; no gradient flows into it.  pairs: sum_s n_s^2 as a host int (it sizes att and checks the prior); without
    it the offsets are read back from the device, which synchronises and cannot be captured in a graph -- the batched
    route passes scene_layout().pairs.  Returns (out (rows, D), att (packed))."""
    pairs = packed_pairs(scene_off) if pairs is None else int(pairs)
    if prior_flat is not None:
        if prior_flat.numel() != pairs:
            raise ValueError("dafm_attention_add: the prior holds %d entries, the scenes' (n, n) blocks %d"
                             % (prior_flat.numel(), pairs))
        prior_flat = prior_flat.detach().reshape(-1).float().contiguous()
    return _DafmAttentionAdd.apply(q.float(), k.float(), v.float(), prior_flat, scene_off, de_off, pairs, scale)
