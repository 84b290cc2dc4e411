"""Inference route of the non-local block (model/backbone.py NLBlockND, mode 'dot'): one launch of csrc/nonlocal_eval.hip per
call -- the three projections, S = G Phi^T / P, Y = S T, W_z, the eval-mode BatchNorm as an affine map and the residual --
instead of four GEMMs, two batched matmuls, a transposing copy, a BatchNorm and an add.  T, Phi, G, S and Y never reach
global memory, and the input is read through its strides, so the RoI-grid head hands over its (n, P, C) rows as they are.

MGAR_NL_EVAL_FUSE=0 (or NL_EVAL_FUSE, for tests) restores the torch route.  Train mode, a required gradient, the other modes
and sizes outside the kernel's envelope (the INTER_PERSON layouts) never leave it."""
import math
import os

import torch
import torch.nn as nn

from . import _lib as L
from .eval_route import bn_frozen, cached, hooked, needs_grad
from .nn_utils import _BN_TYPES, _is_pointwise

NL_EVAL_FUSE = os.environ.get("MGAR_NL_EVAL_FUSE", "1") != "0"
_ENTRY = {torch.float32: "mgar_nonlocal_dot_eval_fwd", torch.bfloat16: "mgar_nonlocal_dot_eval_bf16_fwd"}


def _parts(block):
    """(theta, phi, g, W_z's convolution, W_z's BatchNorm or None) of a 'dot' block built as NLBlockND builds it, else None"""
    wz = block.W_z
    if isinstance(wz, nn.Sequential):
        if len(wz) != 2 or not isinstance(wz[1], _BN_TYPES):
            return None
        conv_z, bn = wz[0], wz[1]
    else:
        conv_z, bn = wz, None
    convs = (getattr(block, "theta", None), getattr(block, "phi", None), block.g, conv_z)
    if not all(c is not None and _is_pointwise(c) for c in convs):
        return None
    ci, c = block.inter_channels, block.in_channels
    if any((m.in_channels, m.out_channels) != (c, ci) for m in convs[:3]) or (conv_z.in_channels, conv_z.out_channels) != (ci, c):
        return None
    return convs + (bn,)


def nl_eval_refusal(block, x, rows=False):
    """Why a call of `block` on x does NOT take the fused kernel -- a short reason -- or None when it does.  x is (n, C, *spatial),
    or (n, P, C) with rows.  Reads nothing but attributes: no device work, no synchronisation."""
    if not NL_EVAL_FUSE:
        return "switch off"
    if block.mode != 'dot':
        return "mode"
    if not torch.is_tensor(x) or x.dtype not in _ENTRY or x.dim() < 3 or (rows and x.dim() != 3):
        return "payload"
    parts = _parts(block)
    if parts is None:
        return "structure"
    bn = parts[4]
    if bn is not None and not bn_frozen(bn):
        return "batch norm"
    if needs_grad(x, block.parameters()):
        return "gradient"
    if hooked(block.W_z, *[m for m in parts if m is not None]):
        return "hook"
    c, p = (x.shape[2], x.shape[1]) if rows else (x.shape[1], math.prod(x.shape[2:]))
    if c != block.in_channels or not L.raw("mgar_nonlocal_dot_eval_supported", c, block.inter_channels, p):
        return "size"
    if not x.is_cuda or any(t.device != x.device for t in block.parameters()):
        return "device"
    return None


def nl_eval_plan(block, x, rows=False):
    """The fused route of `block` on x -- (theta, phi, g, W_z's convolution, W_z's BatchNorm or None) -- or None for the torch route.
    Fused when the switch is on, mode == 'dot', x is a device tensor with fp32 or bf16 payload, the BatchNorm behind W_z (if
    any) is in eval mode with running statistics, nothing needs a gradient (grad mode off, or neither x nor a parameter of the
    block requires one), no forward hook sits on a sub-module and the kernel takes (C, Ci, P)."""
    return _parts(block) if nl_eval_refusal(block, x, rows) is None else None


def _params(block, parts):
    """(w_tpg (3 Ci, C), b_tpg (3 Ci), w_z (C, Ci), b_z (C), scale (C), shift (C)), fp32 on the parameters' device: device ops
    only, no host synchronisation.  Cached on the block (eval_route.cached) under every tensor read, derived from fold_bn's own
    cached pair: a frozen model builds them once, an in-place update of any tensor rebuilds them."""
    from .sparse_ops import fold_bn
    theta, phi, g, conv_z, bn = parts
    read = [m.weight for m in (theta, phi, g, conv_z)] + [m.bias for m in (theta, phi, g, conv_z) if m.bias is not None]
    fold = fold_bn(bn) if bn is not None else (None, None)
    ci, c, dev = block.inter_channels, block.in_channels, conv_z.weight.device

    def bias(m):
        return m.bias.detach().float() if m.bias is not None else torch.zeros(m.out_channels, dtype=torch.float32, device=dev)

    def build():
        w_tpg = torch.cat([m.weight.detach().float().reshape(ci, c) for m in (theta, phi, g)]).contiguous()
        b_tpg = torch.cat([bias(m) for m in (theta, phi, g)]).contiguous()
        w_z, b_z = conv_z.weight.detach().float().reshape(c, ci).contiguous(), bias(conv_z).contiguous()
        scale, shift = fold if bn is not None else (torch.ones(c, dtype=torch.float32, device=dev),
                                                    torch.zeros(c, dtype=torch.float32, device=dev))
        return w_tpg, b_tpg, w_z, b_z, scale, shift
    return cached(block, "_mgar_nl_eval", read, build, derived_from=fold)


def nonlocal_dot_eval_fwd(x, strides, n, c, ci, p, params, z):
    """The C entry point on device tensors: element (a, ch, q) of the input at x.data_ptr() + a strides[0] + ch strides[1] +
    q strides[2] elements; z (n, c, p) contiguous with x's dtype; params the six fp32 tensors of _params."""
    if x.dtype not in _ENTRY or z.dtype != x.dtype:
        raise L.MgarError("nonlocal_dot_eval_fwd: x and z must both be float32 or bfloat16")
    if not x.is_cuda:
        raise L.MgarError("expected a device (HIP) tensor, got %s -- there is no CPU path" % x.device)
    shapes = ((3 * ci, c), (3 * ci,), (c, ci), (c,), (c,), (c,))
    if [tuple(t.shape) for t in params] != list(shapes) or tuple(z.shape) != (n, c, p):
        raise L.MgarError("nonlocal_dot_eval_fwd: parameter or output shapes do not match (n, C, Ci, P)")
    L.call(_ENTRY[x.dtype], x.data_ptr(), int(strides[0]), int(strides[1]), int(strides[2]), n, c, ci, p,
           *[L.fptr(t) for t in params], L.pptr(z, x.dtype), L.stream_of(x))
    return z


def nl_eval_forward(block, x, parts, rows=False):
    """z = block(x) on the fused kernel, for a plan `parts` of nl_eval_plan.  x (n, C, *spatial) -> the same shape; with rows
    x (n, P, C) -> (n, C, P).  Output dtype = input dtype."""
    n = x.shape[0]
    if rows:
        p, c = x.shape[1], x.shape[2]
        strides, out_shape = (x.stride(0), x.stride(2), x.stride(1)), (n, c, p)
    else:
        c, out_shape = x.shape[1], tuple(x.shape)
        p = math.prod(x.shape[2:])
        x = x.reshape(n, c, p)                 # a view wherever the trailing axes can be merged
        strides = x.stride()
    z = torch.empty((n, c, p), dtype=x.dtype, device=x.device)
    if n:
        nonlocal_dot_eval_fwd(x, strides, n, c, block.inter_channels, p, _params(block, parts), z)
    return z.view(out_shape)
