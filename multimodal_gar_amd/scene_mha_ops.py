"""Per-scene multi-head attention over packed scene rows (HIP, csrc/scene_mha.hip): the core of nn.MultiheadAttention
between its projections -- Att = softmax(Q K^T * scale, dim=1), out = Att V for every scene and head -- and
scene_multihead_attention(), which evaluates a whole nn.MultiheadAttention module on the rows of all scenes at once."""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L

HEAD_DIM = 64       # the kernel's one head width (== the wave width)


def _rows_ptr(t):
    """Pointer of a (rows, C) fp32 device tensor whose rows are contiguous but may lie in a wider buffer."""
    if not t.is_cuda:
        raise L.MgarError("expected a device (HIP) tensor, got %s -- there is no CPU path" % t.device)
    if t.dtype != torch.float32:
        raise L.MgarError("expected dtype torch.float32, got %s" % t.dtype)
    return t.data_ptr()


def _common_ld(q, k, v):
    """q, k, v as the kernel takes them: unit column stride, one row stride, 16-byte aligned -- the slices of one fused
    in-projection pass as they are, anything else is copied."""
    def ok(t):
        return t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0
    if not (ok(q) and ok(k) and ok(v) and q.stride(0) == k.stride(0) == v.stride(0)):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return q, k, v, (q.stride(0) if q.shape[0] > 1 else q.shape[1])     # a single row: its stride is never used


class _SceneMHA(Function):
    @staticmethod
    def forward(ctx, q, k, v, scene_off, de_off, pairs, heads, scale):
        rows, width = q.shape
        if width != heads * HEAD_DIM or k.shape != q.shape or v.shape != q.shape:
            raise ValueError("scene_mha: q, k, v must be (rows, %d) for %d heads of %d, got %s %s %s"
                             % (heads * HEAD_DIM, heads, HEAD_DIM, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        q, k, v, ld = _common_ld(q, k, v)
        n_scenes = scene_off.numel() - 1
        att = torch.empty((heads, pairs), dtype=q.dtype, device=q.device)
        out = torch.empty((rows, width), dtype=q.dtype, device=q.device)
        L.call("mgar_scene_mha_fwd", n_scenes, rows, heads, HEAD_DIM, L.iptr(scene_off), L.iptr(de_off), pairs, _rows_ptr(q),
               _rows_ptr(k), _rows_ptr(v), ld, float(scale), L.fptr(att), L.fptr(out), L.stream_of(q))
        ctx.save_for_backward(q, k, v, scene_off, de_off, att)
        ctx.cfg = (pairs, heads, ld, float(scale))
        ctx.mark_non_differentiable(att)      # backward has no gradient path through att
        return out, att

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_att_unused):
        q, k, v, scene_off, de_off, att = ctx.saved_tensors
        pairs, heads, ld, scale = ctx.cfg
        rows, width = q.shape
        gq, gk, gv = (torch.empty((rows, width), dtype=q.dtype, device=q.device) for _ in range(3))
        gmat = torch.empty_like(att)
        grad_out = grad_out.contiguous()
        L.call("mgar_scene_mha_bwd", scene_off.numel() - 1, rows, heads, HEAD_DIM, L.iptr(scene_off), L.iptr(de_off), pairs,
               _rows_ptr(q), _rows_ptr(k), _rows_ptr(v), ld, scale, L.fptr(att), L.fptr(grad_out), L.fptr(gmat), L.fptr(gq),
               L.fptr(gk), L.fptr(gv), L.stream_of(q))
        return gq, gk, gv, None, None, None, None, None


def scene_mha(q, k, v, scene_off, de_off, pairs, heads, scale):
    """q, k, v: (rows, 64 * heads) fp32, rows of all scenes stacked; they may be column slices of one wider buffer (no
    copy then).  pairs = sum_s n_s^2 as a host int (scene_layout().pairs).  -> (out (rows, 64 * heads) contiguous,
    att (heads, pairs), each head's plane packed like de_flat of dafm_attention)."""
    return _SceneMHA.apply(q.float(), k.float(), v.float(), scene_off, de_off, int(pairs), int(heads), scale)


def _check_module(mha):
    """Refuses what the kernel cannot mirror."""
    if mha.embed_dim % mha.num_heads or mha.embed_dim // mha.num_heads != HEAD_DIM:
        raise NotImplementedError("scene_multihead_attention: heads of width %g, the kernel is built for %d"
                                  % (mha.embed_dim / mha.num_heads, HEAD_DIM))
    if mha.dropout != 0 and mha.training:
        raise NotImplementedError("scene_multihead_attention: attention dropout %g in train mode (the kernel draws none)"
                                  % mha.dropout)
    if mha.bias_k is not None or mha.bias_v is not None:
        raise NotImplementedError("scene_multihead_attention: bias_k / bias_v are not supported")
    if mha.add_zero_attn:
        raise NotImplementedError("scene_multihead_attention: add_zero_attn is not supported")
    if not mha._qkv_same_embed_dim or mha.in_proj_weight is None:
        raise NotImplementedError("scene_multihead_attention: separate projection weights (kdim / vdim) are not supported")


def scene_multihead_attention(mha, query, key, value, scene_off, de_off, pairs):
    """`mha(query, key, value)[0]` of an nn.MultiheadAttention called unbatched on every scene's rows, for the packed rows
    (sum_s n_s, embed_dim) of all scenes at once: in_proj as library GEMMs over all rows (one GEMM when query, key and
    value are the same tensor), the attention core in the HIP kernel, out_proj.  fp32 tokens, as dafm_attention."""
    _check_module(mha)
    E, w, b = mha.embed_dim, mha.in_proj_weight, mha.in_proj_bias
    query = query.float()
    if key is query and value is query:
        qkv = F.linear(query, w, b)                                              # (rows, 3E): the slices go in without a copy
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    else:
        def part(x, i):
            return F.linear(x.float(), w[i * E:(i + 1) * E], None if b is None else b[i * E:(i + 1) * E])
        q, k, v = part(query, 0), part(key, 1), part(value, 2)
    out, _ = scene_mha(q, k, v, scene_off, de_off, pairs, mha.num_heads, 1.0 / HEAD_DIM ** 0.5)
    return mha.out_proj(out)
