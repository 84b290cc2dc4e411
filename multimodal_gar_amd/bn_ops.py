"""Fused BatchNorm(training statistics) + ReLU (+ max over nsample) on the HIP kernels of
csrc/bn_act.hip -- the tail of every [Conv 1x1 -> BatchNorm -> ReLU] block of the shared MLPs
(reference pointnet2_batch/pointnet2_modules.py:37-45 and friends).  Parameters and running
statistics live in the caller's ``nn.BatchNormNd`` module, so state dicts are unchanged."""
import os

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L
from .eval_route import bn_frozen, hooked, needs_grad as _needs_grad


def _u8ptr(t):
    return L.dev_ptr(t, torch.uint8)


def _workspace(x, b, c, p):
    return torch.empty((L.raw("mgar_bn_workspace_floats", b, c, p),), dtype=torch.float32, device=x.device)


_PAYLOADS = (torch.float32, torch.bfloat16)   # feature-payload dtypes of the kernels; statistics / affine are always fp32


def _f32(t):
    """BatchNorm vectors (affine, statistics) are fp32 whatever the payload type (a module converted with .to(bf16)
    would otherwise hand bf16 vectors to kernels that read floats)."""
    return t if t is None or t.dtype == torch.float32 else t.float()


STATS_TILE = 128   # columns per statistics partial of the producer kernels (csrc/pointwise_fwd.hip, csrc/query_group.hip)


def stats_partial_buffer(x_like, c, n_per_channel):
    """Buffer a producer kernel fills with the BatchNorm statistics partials of its output -- (C, n / 128, 2): per channel
    and 128-column tile the tile's mean and sum of squared deviations -- or None where that does not apply (n % 128, dtype)."""
    if x_like.dtype != torch.float32 or not x_like.is_cuda or n_per_channel % STATS_TILE != 0 or n_per_channel == 0:
        return None
    return torch.empty((c, n_per_channel // STATS_TILE, 2), dtype=torch.float32, device=x_like.device)


def _train_stats(x3, bn, partial=None):
    b, c, p = x3.shape
    mean = torch.empty((c,), dtype=torch.float32, device=x3.device)
    invstd = torch.empty_like(mean)
    track = bn.track_running_stats and bn.running_mean is not None
    if partial is not None and tuple(partial.shape) == (c, (b * p) // STATS_TILE, 2) and (b * p) % STATS_TILE == 0:
        # the producer of x left the per-tile (mean, M2): merge them, no pass over x (csrc/bn_act.hip, bn_finalize_kernel)
        nws = L.raw("mgar_bn_stats_from_partials_workspace_floats", partial.shape[1], c)
        ws = torch.empty((nws,), dtype=torch.float32, device=x3.device) if nws else None
        L.call("mgar_bn_stats_from_partials", L.fptr(partial), partial.shape[1], c, b * p, STATS_TILE, float(bn.eps),
               float(bn.momentum if bn.momentum is not None else 0.1), L.fptr(ws) if ws is not None else None, L.fptr(mean), L.fptr(invstd),
               L.fptr(bn.running_mean) if track else None, L.fptr(bn.running_var) if track else None,
               L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
               L.stream_of(x3))
        return mean, invstd
    ws = _workspace(x3, b, c, p)
    L.payload_call("mgar_bn_train_stats", x3.dtype, L.pptr(x3, x3.dtype), b, c, p, float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1),
                   L.fptr(ws), L.fptr(mean), L.fptr(invstd), L.fptr(bn.running_mean) if track else None,
                   L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
                   L.stream_of(x3))
    return mean, invstd


ROWMAJOR_GRAD_MAX_CHANNELS = 64   # csrc/bn_act.hip: bn_bwd_apply_t_kernel transposes through a 64 x 65 LDS tile


def _bwd_rowmajor(dy, x3, mean, invstd, gamma, beta, relu, ws, dgamma, dbeta):
    """BatchNorm [+ ReLU] backward whose input gradient is stored ROW-MAJOR, (B * P, C), and handed to autograd as the
    (B, C, P) transposed VIEW of that memory: the consumer that asked for it (the atomic-free stacked grouping backward,
    pointnet2_stack/pointnet2_utils.py) reads whole rows; anything else sees an ordinary strided tensor."""
    b, c, p = x3.shape
    dx_t = torch.empty((b, p, c), dtype=torch.float32, device=x3.device)
    L.call("mgar_bn_act_bwd_rowmajor", L.fptr(dy), L.fptr(x3), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
           int(relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(dx_t), L.stream_of(x3))
    return dx_t.permute(0, 2, 1)


class _BnAct(Function):
    """y = [relu](batch_norm_train(x)) for x (B, C, P); saves x (not y) for the backward."""

    @staticmethod
    def forward(ctx, x3, gamma, beta, mean, invstd, relu, rowmajor_grad=False):
        b, c, p = x3.shape
        ctx.rowmajor = bool(rowmajor_grad) and x3.dtype == torch.float32 and c <= ROWMAJOR_GRAD_MAX_CHANNELS
        y = torch.empty_like(x3)
        dt = x3.dtype
        L.payload_call("mgar_bn_act_fwd", dt, L.pptr(x3, dt), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                       int(relu), L.pptr(y, dt), L.stream_of(x3))
        ctx.save_for_backward(x3, gamma, beta, mean, invstd)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x3, gamma, beta, mean, invstd = ctx.saved_tensors
        b, c, p = x3.shape
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        # every tensor whose pointer is passed stays bound to a name until the call returns: a
        # temporary freed mid-expression can be handed out again by the caching allocator
        dt = x3.dtype
        dy_c, ws = dy.contiguous().to(dt), _workspace(x3, b, c, p)
        if ctx.rowmajor:
            return _bwd_rowmajor(dy_c, x3, mean, invstd, gamma, beta, ctx.relu, ws, dgamma, dbeta), dgamma, dbeta, None, None, None, None
        dx = torch.empty_like(x3)
        L.payload_call("mgar_bn_act_bwd", dt, L.pptr(dy_c, dt), L.pptr(x3, dt), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
                       L.fptr(beta), int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.pptr(dx, dt), L.stream_of(x3))
        return dx, dgamma, dbeta, None, None, None, None


class _BnActMaxPool(Function):
    """pooled (B, C, M) = max_s [relu](batch_norm_train(x))[b, c, m, s] for x (B, C, M, ns)."""

    @staticmethod
    def forward(ctx, x4, gamma, beta, mean, invstd, relu):
        b, c, m, ns = x4.shape
        dt = x4.dtype
        out = torch.empty((b, c, m), dtype=dt, device=x4.device)
        arg = torch.empty((b, c, m), dtype=torch.uint8, device=x4.device)
        xarg = torch.empty((b, c, m), dtype=dt, device=x4.device) if x4.requires_grad or gamma.requires_grad else None
        L.payload_call("mgar_bn_act_maxpool_fwd", dt, L.pptr(x4, dt), b, c, m, ns, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
                       L.fptr(beta), int(relu), L.pptr(out, dt), _u8ptr(arg), L.pptr(xarg, dt) if xarg is not None else None,
                       L.stream_of(x4))
        ctx.save_for_backward(x4, gamma, mean, invstd, out, arg, xarg)
        ctx.relu = bool(relu)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, dpool, darg=None):
        x4, gamma, mean, invstd, out, arg, xarg = ctx.saved_tensors
        b, c, m, ns = x4.shape
        dx = torch.empty_like(x4)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        dt = x4.dtype
        ws = _workspace(x4, b, c, m * ns)
        if dt == torch.float32 and dpool.dtype == dt and dpool.dim() == 3 and not dpool.is_contiguous() \
                and (b == 1 or dpool.stride(0) >= 0) and min(dpool.stride(1), dpool.stride(2)) >= 1:
            # a channel slice of the concatenated scales, or the transposed view of (M, C_total) rows: read in place
            L.call("mgar_bn_act_maxpool_bwd_strided", dpool.data_ptr(), dpool.stride(0) if b > 1 else 0, dpool.stride(1), dpool.stride(2),
                   L.fptr(out), _u8ptr(arg), L.fptr(x4), L.fptr(xarg) if xarg is not None else None, b, c, m, ns, L.fptr(mean),
                   L.fptr(invstd), L.fptr(gamma), int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(dx), L.stream_of(x4))
            return dx, dgamma, dbeta, None, None, None
        dpool_c = dpool.contiguous().to(dt)
        L.payload_call("mgar_bn_act_maxpool_bwd", dt, L.pptr(dpool_c, dt), L.pptr(out, dt), _u8ptr(arg), L.pptr(x4, dt),
                       L.pptr(xarg, dt) if xarg is not None else None, b, c, m, ns, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
                       int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.pptr(dx, dt), L.stream_of(x4))
        return dx, dgamma, dbeta, None, None, None


class _BnActConv(Function):
    """y = W . [relu](batch_norm_train(x)) for x (B, C, P), W (Cout, C): one [BN -> ReLU -> Conv 1x1] step of
    a shared MLP on csrc/pointwise_fwd.hip.  The activated tensor is never written: the forward
    applies BN + ReLU to x while feeding the MFMA, the backward recomputes it inside the weight-
    gradient kernel (csrc/pointwise_dw.hip); only the pre-BN x is saved."""

    @staticmethod
    def forward(ctx, x3, gamma, beta, mean, invstd, relu, w, rowmajor_grad=False, out_stats=None):
        """out_stats (optional, stats_partial_buffer(y)): filled with the statistics partials of y for the BatchNorm that follows."""
        b, c, p = x3.shape
        ctx.rowmajor = bool(rowmajor_grad) and x3.dtype == torch.float32 and c <= ROWMAJOR_GRAD_MAX_CHANNELS
        cout = w.shape[0]
        w = w.contiguous()
        dt = x3.dtype
        y = torch.empty((b, cout, p), dtype=dt, device=x3.device)
        if out_stats is not None:
            L.call("mgar_pointwise_conv_fwd_stats", L.fptr(x3), b, c, p, L.fptr(w), c, 1, cout, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), L.fptr(y), L.fptr(out_stats), L.stream_of(x3))
        else:
            L.payload_call("mgar_pointwise_conv_fwd", dt, L.pptr(x3, dt), b, c, p, L.fptr(w), c, 1, cout, L.fptr(mean), L.fptr(invstd),
                           L.fptr(gamma), L.fptr(beta), int(relu), L.pptr(y, dt), L.stream_of(x3))
        ctx.save_for_backward(x3, gamma, beta, mean, invstd, w)
        ctx.relu = relu
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x3, gamma, beta, mean, invstd, w = ctx.saved_tensors
        b, c, p = x3.shape
        cout = w.shape[0]
        gy = gy.contiguous()
        st = L.stream_of(x3)
        # grad wrt the activated input: W^T gy (the forward kernel, W read transposed, no activation)
        ga = torch.empty_like(x3)
        L.call("mgar_pointwise_conv_fwd", L.fptr(gy), b, cout, p, L.fptr(w), 1, c, c, None, None, None, None, 0,
               L.fptr(ga), st)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        if FUSED_DW_BN_REDUCE and ctx.needs_input_grad[6]:
            # dW and the BatchNorm backward's reduction {sum dz, sum dz xhat} from ONE pass over (x, gy) on the matrix cores
            # (csrc/pointwise_dw.hip, pair mode): no reduction pass over (W^T gy, x); then the apply pass alone
            dw = torch.empty_like(w)
            coef = torch.empty((2 * c,), dtype=torch.float32, device=x3.device)
            wsd = torch.empty((max(1, L.raw("mgar_pointwise_dw_bnbwd_workspace_floats", b, c, cout, p)),), dtype=torch.float32,
                              device=x3.device)
            L.call("mgar_pointwise_conv_dw_bnbwd", L.fptr(x3), L.fptr(gy), L.fptr(w), b, c, cout, p, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(ctx.relu), L.fptr(wsd), L.fptr(dw), L.fptr(dgamma), L.fptr(dbeta), L.fptr(coef), st)
            dx = torch.empty((b, p, c) if ctx.rowmajor else (b, c, p), dtype=torch.float32, device=x3.device)
            L.call("mgar_bn_act_bwd_apply", L.fptr(ga), L.fptr(x3), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                   int(ctx.relu), L.fptr(coef), int(ctx.rowmajor), L.fptr(dx), st)
            return (dx.permute(0, 2, 1) if ctx.rowmajor else dx), dgamma, dbeta, None, None, None, dw, None, None
        dw = None
        if ctx.needs_input_grad[6]:
            dw = torch.empty_like(w)
            wsd = torch.empty((max(1, L.raw("mgar_pointwise_dw_workspace_floats", b, c, cout, p)),), dtype=torch.float32,
                              device=x3.device)
            L.call("mgar_pointwise_conv_dw_act", L.fptr(x3), L.fptr(gy), b, c, cout, p, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(ctx.relu), L.fptr(wsd), L.fptr(dw), st)
        ws = _workspace(x3, b, c, p)
        if ctx.rowmajor:
            return _bwd_rowmajor(ga, x3, mean, invstd, gamma, beta, ctx.relu, ws, dgamma, dbeta), dgamma, dbeta, None, None, None, dw, None, None
        dx = torch.empty_like(x3)
        L.call("mgar_bn_act_bwd", L.fptr(ga), L.fptr(x3), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
               L.fptr(beta), int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(dx), st)
        return dx, dgamma, dbeta, None, None, None, dw, None, None


class _BnActConvBnMaxPool(Function):
    """pooled (B, Ck, M) = max_s relu2?(bn2(W . relu?(bn(x))))[b, :, m, s] for x (B, C, M * ns): the last two layers of a shared
    MLP, [BN -> ReLU -> Conv 1x1] and [BN -> ReLU -> max over ns], as ONE autograd node.  The forward issues the launches of
    _BnActConv followed by _BnActMaxPool.  The backward never writes the max-pool layer's input gradient (the widest tensor
    of the module): after the reduction half of the max-pool backward, the conv's dX and dW kernels form it in their operand
    prologues from the saved pre-BN tensor (csrc/pointwise_fwd.hip GRAD mode, csrc/pointwise_dw.hip GRAD instances) -- one
    read and one write of that tensor less, bit for bit the same products."""

    @staticmethod
    def forward(ctx, x3, gamma, beta, mean, invstd, relu, w, gamma2, beta2, bn2, relu2, m, ns, rowmajor_grad=False):
        b, c, p = x3.shape
        ctx.rowmajor = bool(rowmajor_grad) and c <= ROWMAJOR_GRAD_MAX_CHANNELS
        ck = w.shape[0]
        w = w.contiguous()
        st = L.stream_of(x3)
        x4 = torch.empty((b, ck, m, ns), dtype=torch.float32, device=x3.device)
        out_stats = stats_partial_buffer(x3, ck, b * p) if ck <= FUSED_STATS_MAX_CHANNELS and p % STATS_TILE == 0 else None
        if out_stats is not None:
            L.call("mgar_pointwise_conv_fwd_stats", L.fptr(x3), b, c, p, L.fptr(w), c, 1, ck, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), L.fptr(x4), L.fptr(out_stats), st)
        else:
            L.call("mgar_pointwise_conv_fwd", L.fptr(x3), b, c, p, L.fptr(w), c, 1, ck, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), L.fptr(x4), st)
        mean2, invstd2 = _train_stats(x4.view(b, ck, p), bn2, out_stats)
        out = torch.empty((b, ck, m), dtype=torch.float32, device=x3.device)
        arg = torch.empty((b, ck, m), dtype=torch.uint8, device=x3.device)
        xarg = torch.empty((b, ck, m), dtype=torch.float32, device=x3.device) if any(ctx.needs_input_grad) else None
        L.call("mgar_bn_act_maxpool_fwd", L.fptr(x4), b, ck, m, ns, L.fptr(mean2), L.fptr(invstd2), L.fptr(gamma2), L.fptr(beta2),
               int(relu2), L.fptr(out), _u8ptr(arg), L.fptr(xarg) if xarg is not None else None, st)
        ctx.save_for_backward(x3, gamma, beta, mean, invstd, w, x4, gamma2, mean2, invstd2, out, arg, xarg)
        ctx.relu, ctx.relu2 = bool(relu), bool(relu2)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dpool):
        x3, gamma, beta, mean, invstd, w, x4, gamma2, mean2, invstd2, out, arg, xarg = ctx.saved_tensors
        b, c, p = x3.shape
        _, ck, m, ns = x4.shape
        st = L.stream_of(x3)
        dev = x3.device
        # 1. reduction half of the max-pool layer's BatchNorm backward: coef2 = {mean dz, mean dz xhat}, and the masked pooled
        #    gradient as a contiguous (B, Ck, M) array whatever the layout dpool came in
        dgamma2, dbeta2 = torch.empty_like(gamma2), torch.empty_like(gamma2)
        coef2 = torch.empty((2 * ck,), dtype=torch.float32, device=dev)
        dmask = torch.empty((b, ck, m), dtype=torch.float32, device=dev)
        ws2 = _workspace(x4, b, ck, p)
        if dpool.dtype == torch.float32 and dpool.dim() == 3 and not dpool.is_contiguous() \
                and (b == 1 or dpool.stride(0) >= 0) and min(dpool.stride(1), dpool.stride(2)) >= 1:
            # a channel slice of the concatenated scales, or the transposed view of (M, C_total) rows: read in place
            dp, strides = dpool, (dpool.stride(0) if b > 1 else 0, dpool.stride(1), dpool.stride(2))
        else:
            dp, strides = dpool.contiguous().float(), (0, -1, 1)
        L.call("mgar_bn_act_maxpool_bwd_reduce", dp.data_ptr(), strides[0], strides[1], strides[2], L.fptr(out), _u8ptr(arg),
               L.fptr(x4), L.fptr(xarg) if xarg is not None else None, b, ck, m, ns, L.fptr(mean2), L.fptr(invstd2),
               int(ctx.relu2), L.fptr(ws2), L.fptr(dgamma2), L.fptr(dbeta2), L.fptr(coef2), L.fptr(dmask), st)
        # 2. grad wrt the conv's activated input, W^T dx4, with dx4 formed from x4 in the operand prologue
        ga = torch.empty_like(x3)
        L.call("mgar_pointwise_conv_fwd_maxgrad", L.fptr(x4), b, ck, m, ns, L.fptr(w), 1, c, c, L.fptr(mean2), L.fptr(invstd2),
               L.fptr(gamma2), L.fptr(coef2), _u8ptr(arg), L.fptr(dmask), L.fptr(ga), st)
        # 3. dW the same way (the X operand keeps its own activation recompute)
        dw = None
        if ctx.needs_input_grad[6]:
            dw = torch.empty_like(w)
            wsd = torch.empty((max(1, L.raw("mgar_pointwise_dw_workspace_floats", b, c, ck, p)),), dtype=torch.float32, device=dev)
            L.call("mgar_pointwise_conv_dw_maxgrad", L.fptr(x3), L.fptr(x4), b, c, ck, m, ns, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(ctx.relu), L.fptr(mean2), L.fptr(invstd2), L.fptr(gamma2), L.fptr(coef2),
                   _u8ptr(arg), L.fptr(dmask), L.fptr(wsd), L.fptr(dw), st)
        # 4. the inner BatchNorm [+ ReLU] backward, as in _BnActConv
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        ws = _workspace(x3, b, c, p)
        if ctx.rowmajor:
            dx = _bwd_rowmajor(ga, x3, mean, invstd, gamma, beta, ctx.relu, ws, dgamma, dbeta)
        else:
            dx = torch.empty_like(x3)
            L.call("mgar_bn_act_bwd", L.fptr(ga), L.fptr(x3), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma),
                   L.fptr(beta), int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(dx), st)
        return dx, dgamma, dbeta, None, None, None, dw, dgamma2, dbeta2, None, None, None, None, None


class _PlainConv(Function):
    """y = W x for the FIRST layer of a shared MLP (no BatchNorm in front of it): csrc/pointwise_fwd.hip with the identity in
    place of the activation, so the output is written once at streaming rate and -- when a BatchNorm follows -- the kernel
    leaves that BatchNorm's statistics partials behind (no statistics pass over the widest tensor of the module)."""

    @staticmethod
    def forward(ctx, x3, w, out_stats=None):
        b, c, p = x3.shape
        cout = w.shape[0]
        w = w.contiguous()
        dt = x3.dtype
        y = torch.empty((b, cout, p), dtype=dt, device=x3.device)
        if out_stats is not None:
            L.call("mgar_pointwise_conv_fwd_stats", L.fptr(x3), b, c, p, L.fptr(w), c, 1, cout, None, None, None, None, 0,
                   L.fptr(y), L.fptr(out_stats), L.stream_of(x3))
        else:
            L.payload_call("mgar_pointwise_conv_fwd", dt, L.pptr(x3, dt), b, c, p, L.fptr(w), c, 1, cout, None, None, None, None, 0,
                           L.pptr(y, dt), L.stream_of(x3))
        ctx.save_for_backward(x3, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x3, w = ctx.saved_tensors
        b, c, p = x3.shape
        cout = w.shape[0]
        gy = gy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x3)
            L.call("mgar_pointwise_conv_fwd", L.fptr(gy), b, cout, p, L.fptr(w), 1, c, c, None, None, None, None, 0, L.fptr(dx),
                   L.stream_of(x3))
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            wsd = torch.empty((max(1, L.raw("mgar_pointwise_dw_workspace_floats", b, c, cout, p)),), dtype=torch.float32,
                              device=x3.device)
            L.call("mgar_pointwise_conv_dw", L.fptr(x3), L.fptr(gy), b, c, cout, p, L.fptr(wsd), L.fptr(dw), L.stream_of(x3))
        return dx, dw, None


PLAIN_CONV_MAX_OUT = 32      # one 32-row output block (csrc/pointwise_fwd.hip OB = 1): above it the library GEMM is as fast
PLAIN_CONV_MAX_IN = 32


def plain_conv(x, conv, want_out_stats=False, bf16_mfma=False):
    """conv(x) for a bias-free kernel-size-1 ``conv`` that has no BatchNorm in front (the first layer of a shared MLP), or None
    outside the kernel's shapes (the caller takes the library GEMM).  -> y, or (y, statistics partials | None).  ``bf16_mfma``:
    the caller's consent to the bf16-MFMA kernel for bf16 payloads (mlp_bf16_mfma_plan); PointwiseSequential withholds it where
    an eval-mode BatchNorm follows (the inference route keeps its kernels)."""
    if not (x.is_cuda and x.dtype in _PAYLOADS and x.dim() >= 3 and conv.bias is None):
        return None
    if x.dtype != torch.float32 and _needs_grad(x, (conv.weight,)):
        return None
    c, cout = x.shape[1], conv.out_channels
    x3 = x.contiguous().flatten(2)
    if c > PLAIN_CONV_MAX_IN or cout > PLAIN_CONV_MAX_OUT or x3.shape[2] % 4 != 0 or x3.shape[0] * x3.shape[2] < (1 << 16):
        return None
    needs_grad = _needs_grad(x, (conv.weight,))
    if bf16_mfma and mlp_bf16_mfma_plan(x3, cout, needs_grad, None, PLAIN_CONV_MAX_IN, PLAIN_CONV_MAX_OUT):
        y = _conv_bf16_mfma(x3, _f32(conv.weight.detach()).view(cout, c), None, None, None, None, False)
        y = y.view(x.shape[0], cout, *x.shape[2:])
        return (y, None) if want_out_stats else y   # bf16 has no statistics epilogue (stats_partial_buffer)
    out_stats = stats_partial_buffer(x3, cout, x3.shape[0] * x3.shape[2]) if want_out_stats and x3.shape[2] % STATS_TILE == 0 else None
    y = _PlainConv.apply(x3, _f32(conv.weight).view(cout, c), out_stats).view(x.shape[0], cout, *x.shape[2:])
    return (y, out_stats) if want_out_stats else y


# _BnActConv.backward: dW and the BatchNorm-backward reduction from one pass (csrc/pointwise_dw.hip, pair mode) instead of dW,
# then reduce + apply.  Measured at c3 (round 2): bn_bwd_partial 7.3 -> 3.4 ms per step, but pointwise_dw 6.5 -> 12.6 ms -- the
# dW kernel is bound by its LDS staging and operand reads, not by HBM, so doubling its (virtual) input channels doubles its
# time: 228.7 -> 232.5 ms per step.  Kept (tested, tests/test_fused_stats_gpu.py) but off.
FUSED_DW_BN_REDUCE = False
FUSED_CONV_MAX_CHANNELS = 64   # csrc/pointwise_fwd.hip: Cout <= 64 in both directions


FUSED_STATS_MAX_CHANNELS = 32   # csrc/pointwise_fwd.hip: the statistics epilogue exists for Cout <= 32


# bf16 payloads that need no gradient take the bf16-MFMA forward kernel (csrc/pointwise_bf16.hip, mgar_pointwise_mfma_bf16_fwd)
# in the train-mode / no-prologue steps of the shared MLPs -- bn_act_conv and plain_conv, inside their own shape gates -- where
# mgar_pointwise_conv_fwd_bf16 widens every element and multiplies on the fp32 MFMA.  The activated input and the weight are
# rounded to bf16 there (two roundings the widening route does not have).  MGAR_MLP_BF16_MFMA=0 (or this
# flag) restores the widening route (A/B in tests and profiles).  The inference route (eval_mlp_plan) is not touched.
MLP_BF16_MFMA = os.environ.get("MGAR_MLP_BF16_MFMA", "1") != "0"


def mlp_bf16_mfma_plan(x, cout, needs_grad, bn=None, max_in=FUSED_CONV_MAX_CHANNELS, max_out=FUSED_CONV_MAX_CHANNELS):
    """True where conv(relu?(bn(x))) -- ``bn`` None: conv(x) -- goes to mgar_pointwise_mfma_bf16_fwd.  Decided from attributes
    alone (x.dtype, x.is_cuda, x.shape, bn.training, the caller's ``needs_grad``, the switch): no tensor is read, nothing
    synchronises.  All of: the switch is on; x is a bf16 device tensor (B, C, ...); no gradient is needed; the BatchNorm, if
    any, is in training mode (the inference route keeps its kernels); 1 <= C <= max_in, 1 <= Cout <= max_out (the caller's
    gates: 64 / 64 for bn_act_conv, 32 / 32 for plain_conv); P % 4 == 0; B * P >= 65 536."""
    if not (MLP_BF16_MFMA and x.dtype == torch.bfloat16 and x.is_cuda and len(x.shape) >= 3) or needs_grad:
        return False
    if bn is not None and not bn.training:
        return False
    c, p = x.shape[1], 1
    for s in x.shape[2:]:
        p *= s
    return 1 <= c <= max_in and 1 <= cout <= max_out and p % 4 == 0 and x.shape[0] * p >= EVAL_MIN_COLUMNS


def _conv_bf16_mfma(x3, w, mean, invstd, gamma, beta, relu):
    """x3 (B, C, P) bf16, w (Cout, C) fp32 -> (B, Cout, P) bf16 on csrc/pointwise_bf16.hip; mean None: no prologue.  No autograd
    node: the callers take it only where no gradient is needed."""
    b, c, p = x3.shape
    cout = w.shape[0]
    w = w.contiguous()
    y = torch.empty((b, cout, p), dtype=torch.bfloat16, device=x3.device)
    L.call("mgar_pointwise_mfma_bf16_fwd", L.pptr(x3, torch.bfloat16), b, c, p, L.fptr(w), c, 1, cout, L.fptr(mean), L.fptr(invstd),
           L.fptr(gamma), L.fptr(beta), int(relu), L.pptr(y, torch.bfloat16), L.stream_of(x3))
    return y


# Inference (every BatchNorm on running statistics, no gradient) keeps the shared MLPs on csrc/pointwise_fwd.hip: a hidden
# [BN -> ReLU -> conv] step is mgar_pointwise_conv_fwd with the running statistics, and the tail [BN -> ReLU ->] conv -> BN
# [-> ReLU] -> max over nsample is ONE launch of mgar_pointwise_conv_maxpool_eval_fwd / _bf16_fwd, which never writes the
# conv's output.  MGAR_MLP_EVAL_FUSE=0 (or this flag) restores bn_act + library GEMM + bn_act_maxpool (A/B in tests, profiles).
MLP_EVAL_FUSE = os.environ.get("MGAR_MLP_EVAL_FUSE", "1") != "0"
EVAL_POOL_NSAMPLES = (4, 8, 16, 32, 64, 128)   # csrc/pointwise_fwd.hip MAXPOOL epilogue: groups lane-aligned in a 128-column tile
EVAL_POOL_MAX_IN = 256                         # mgar_pointwise_conv_maxpool_eval_fwd: 1 <= Cin <= 256, Cout <= 64
EVAL_MIN_COLUMNS = 1 << 16                     # the threshold of every fused kernel of this file


def eval_mlp_plan(x, bn, conv, bn2=None, others=()):
    """Which inference kernel takes conv(relu?(bn(x))) -- "conv" -- or, with ``bn2``, max over the last axis of
    relu?(bn2(conv(relu?(bn(x))))) -- "conv_maxpool"; None = neither (the caller keeps its other route).  ``bn`` None: the conv
    reads x itself.  ``others``: further modules the fused step swallows (the ReLUs).  Decided from attributes alone -- no tensor
    is read, nothing synchronises: the switch is on; x is a device tensor, fp32 or bf16; every BatchNorm is in eval mode with
    running statistics; the conv is point-wise and bias-free; no gradient is required (grad mode off, or neither x nor a
    parameter of these layers requires one); no forward (pre-)hook sits on these layers; B * P >= 65 536 columns; and the shapes
    are the kernels': "conv" C, Cout <= 64 and P % 4 == 0, "conv_maxpool" x (B, C, M, ns) with ns in {4, .., 128}, C <= 256,
    Cout <= 64."""
    from .nn_utils import _BN_TYPES, _is_pointwise
    if not (MLP_EVAL_FUSE and x.is_cuda and x.dtype in _PAYLOADS and x.dim() >= 3):
        return None
    mods = [m for m in (bn, conv, bn2) + tuple(others) if m is not None]
    for m in (bn, bn2):
        if m is not None and not (isinstance(m, _BN_TYPES) and m.track_running_stats and bn_frozen(m)):
            return None
    if not _is_pointwise(conv) or conv.bias is not None:
        return None
    if _needs_grad(x, (p for m in mods for p in m.parameters(recurse=False))):
        return None
    if hooked(*mods):
        return None
    c, cout = x.shape[1], conv.out_channels
    if conv.in_channels != c or c < 1 or (bn is not None and bn.num_features != c) or (bn2 is not None and bn2.num_features != cout):
        return None
    columns = x.shape[0]
    for s in x.shape[2:]:
        columns *= s
    if columns < EVAL_MIN_COLUMNS:
        return None
    if bn2 is not None:
        ok = x.dim() == 4 and x.shape[3] in EVAL_POOL_NSAMPLES and c <= EVAL_POOL_MAX_IN and cout <= FUSED_CONV_MAX_CHANNELS
        return "conv_maxpool" if ok else None
    if bn is None or c > FUSED_CONV_MAX_CHANNELS or cout > FUSED_CONV_MAX_CHANNELS or (columns // x.shape[0]) % 4 != 0:
        return None
    return "conv"


def bn_act_conv_maxpool_eval(x, bn, relu, conv, bn2, relu2, others=()):
    """Inference: max over the last axis of relu2?(bn2(conv(relu?(bn(x))))) for x (B, C, M, ns) -> (B, Ck, M) as one launch
    (csrc/pointwise_fwd.hip, MAXPOOL epilogue), or None where eval_mlp_plan refuses.  ``bn`` None: conv(x) with no prologue (an
    MLP whose only conv is its first layer).  bn2 enters as the float64-folded (scale, shift) of sparse_ops.fold_bn, cached
    on the module."""
    if eval_mlp_plan(x, bn, conv, bn2, others) != "conv_maxpool":
        return None
    from .sparse_ops import fold_bn
    b, c, m, ns = x.shape
    ck = conv.out_channels
    dt = x.dtype
    x4 = x.contiguous()
    w = _f32(conv.weight.detach()).reshape(ck, c).contiguous()
    scale, shift = fold_bn(bn2)
    mean = invstd = gamma = beta = None
    if bn is not None:
        mean, invstd = _stats(x4, bn)
        gamma, beta = _affine(bn, c, x.device)
        gamma, beta = gamma.detach(), beta.detach()
    out = torch.empty((b, ck, m), dtype=dt, device=x.device)
    L.call("mgar_pointwise_conv_maxpool_eval_fwd" if dt == torch.float32 else "mgar_pointwise_conv_maxpool_eval_bf16_fwd",
           L.pptr(x4, dt), b, c, m, ns, L.fptr(w), c, 1, ck, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta), int(relu),
           L.fptr(scale), L.fptr(shift), int(relu2), L.pptr(out, dt), L.stream_of(x4))
    return out


def _bn_act_conv_eval(x, bn, relu, conv, others):
    """Inference [BN -> ReLU -> conv] on mgar_pointwise_conv_fwd with the running statistics: no statistics epilogue, no
    autograd node."""
    if eval_mlp_plan(x, bn, conv, None, others) != "conv":
        return None
    c, cout = x.shape[1], conv.out_channels
    x3 = x.contiguous().flatten(2)
    b, _, p = x3.shape
    dt = x3.dtype
    mean, invstd = _stats(x3, bn)
    gamma, beta = _affine(bn, c, x.device)
    gamma, beta = gamma.detach(), beta.detach()
    w = _f32(conv.weight.detach()).reshape(cout, c).contiguous()
    y = torch.empty((b, cout, p), dtype=dt, device=x.device)
    L.payload_call("mgar_pointwise_conv_fwd", dt, L.pptr(x3, dt), b, c, p, L.fptr(w), c, 1, cout, L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), L.pptr(y, dt), L.stream_of(x3))
    return y.view(x.shape[0], cout, *x.shape[2:])


# bf16 payloads that need no gradient take csrc/pointwise_wide_bf16.hip in the shared-MLP layers with MORE than 64 channels on
# either side (SA levels 2-4, the FP modules, the FP projections): [BN -> ReLU ->] conv as one launch where the route above runs
# the statistics pass, mgar_bn_act_fwd_bf16 and a batched library GEMM, and in eval mode the tail [BN -> ReLU ->] conv -> BN
# [-> ReLU] [-> max over nsample] as one launch.  Every shape the narrow kernels or plain_conv take
# stays where it is.  MGAR_MLP_BF16_WIDE (or this flag) switches it; MGAR_MLP_EVAL_FUSE=0 switches its eval-mode forms off too.
MLP_BF16_WIDE = os.environ.get("MGAR_MLP_BF16_WIDE", "1") != "0"
WIDE_MAX_IN, WIDE_MAX_OUT = 1024, 512          # mgar_pointwise_wide_bf16_fwd: 1 <= Cin <= 1024, 1 <= Cout <= 512
# The plan is NARROWER than the kernel.  Per shape (profiles/README.md, tools/pointwise_wide_bf16.py) the kernel beats bn_act +
# library GEMM [+ bn_act_maxpool] by 1.26 - 2.5x wherever both channel counts are at most 128 and loses from Cin = 196 up (0.34 -
# 0.82x: G waves re-read the x tile through the L1, which is the limit there, not HBM); 128 -> 196 and 96 -> 256 are a draw.
# So the host routes the kernel up to 128 / 128 and everything wider keeps the library GEMM.  Tests lift the two gates.
WIDE_PLAN_MAX_IN, WIDE_PLAN_MAX_OUT = 128, 128
WIDE_FWD, WIDE_POOL = "mgar_pointwise_wide_bf16_fwd", "mgar_pointwise_wide_maxpool_bf16_fwd"


def mlp_bf16_wide_plan(x, conv, bn=None, bn2=None, others=(), pool=False, cin=None):
    """True where bn2?(conv(relu?(bn(x)))) [-> max over the last axis: ``pool``] goes to csrc/pointwise_wide_bf16.hip.  ``bn``
    None: the conv reads x itself; ``bn2`` None: the plain store; ``others``: further modules the step swallows (the ReLUs);
    ``cin``: the conv applies a column slice of its weight to x's ``cin`` channels (the FP projections).  Decided from
    attributes alone -- no tensor is read, nothing synchronises.  All of: the switch is on; x is a bf16 device tensor
    (B, C, ...); no gradient is required (grad mode off, or neither x nor a parameter of these layers requires one); the conv
    is point-wise and bias-free; max(C, Cout) > 64 (everything else stays on the narrow kernels); C <= 1024, Cout <= 512 (the
    kernel's limits) and C <= WIDE_PLAN_MAX_IN, Cout <= WIDE_PLAN_MAX_OUT (128 / 128: where the kernel was measured to win);
    P % 4 == 0; B * P >= 65 536; no forward (pre-)hook on these layers; every eval-mode BatchNorm has running statistics and
    MLP_EVAL_FUSE is on; bn2 is in eval mode; ``pool``: x (B, C, M, ns) with ns in EVAL_POOL_NSAMPLES and a bn2; the library
    has the symbol."""
    from .nn_utils import _BN_TYPES, _is_pointwise
    if not (MLP_BF16_WIDE and x.dtype == torch.bfloat16 and x.is_cuda and len(x.shape) >= 3):
        return False
    if (WIDE_POOL if pool else WIDE_FWD) not in L._fns:
        return False
    mods = [m for m in (bn, conv, bn2) + tuple(others) if m is not None]
    for m in (bn, bn2):
        if m is None:
            continue
        if not isinstance(m, _BN_TYPES):
            return False
        if not m.training and not (MLP_EVAL_FUSE and m.track_running_stats and bn_frozen(m)):
            return False
    if bn2 is not None and bn2.training:
        return False
    if not _is_pointwise(conv) or conv.bias is not None:
        return False
    if _needs_grad(x, (p for m in mods for p in m.parameters(recurse=False))):
        return False
    if hooked(*mods):
        return False
    c, cout = x.shape[1], conv.out_channels
    if (conv.in_channels != c if cin is None else cin != c) or (bn is not None and bn.num_features != c) \
            or (bn2 is not None and bn2.num_features != cout):
        return False
    if max(c, cout) <= FUSED_CONV_MAX_CHANNELS or not (1 <= c <= WIDE_MAX_IN and 1 <= cout <= WIDE_MAX_OUT):
        return False
    if c > WIDE_PLAN_MAX_IN or cout > WIDE_PLAN_MAX_OUT:
        return False
    p = 1
    for s in x.shape[2:]:
        p *= s
    if p % 4 != 0 or x.shape[0] * p < EVAL_MIN_COLUMNS:
        return False
    if pool and not (bn2 is not None and len(x.shape) == 4 and x.shape[3] in EVAL_POOL_NSAMPLES):
        return False
    return True


def _wide_launch(x3, w, w_ld, cout, pro, relu, epi, relu2, ns=0):
    """x3 (B, C, P) bf16 contiguous; w: fp32 device tensor whose element (o, i) lies w_ld * o + i floats behind its data pointer;
    pro = (mean, invstd, gamma, beta) | None; epi = (scale, shift) | None; ns: the pooled entry.  No autograd node."""
    b, c, p = x3.shape
    mean, invstd, gamma, beta = pro if pro is not None else (None,) * 4
    scale, shift = epi if epi is not None else (None, None)
    if w.dtype != torch.float32 or not w.is_cuda:
        raise L.MgarError("the wide bf16 kernel takes an fp32 device weight")
    xp, st = L.pptr(x3, torch.bfloat16), L.stream_of(x3)
    if ns:
        y = torch.empty((b, cout, p // ns), dtype=torch.bfloat16, device=x3.device)
        L.call(WIDE_POOL, xp, b, c, p // ns, ns, w.data_ptr(), w_ld, cout, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
               int(relu), L.fptr(scale), L.fptr(shift), int(relu2), L.pptr(y, torch.bfloat16), st)
    else:
        y = torch.empty((b, cout, p), dtype=torch.bfloat16, device=x3.device)
        L.call(WIDE_FWD, xp, b, c, p, w.data_ptr(), w_ld, cout, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
               int(relu), L.fptr(scale), L.fptr(shift), int(relu2), L.pptr(y, torch.bfloat16), cout * p, st)
    return y


def conv_bf16_wide(x, conv, bn=None, relu=False, bn2=None, relu2=False, pool=False, others=(), in_stats=None, cols=None):
    """bn2?(conv(relu?(bn(x)))) [-> max over the last axis] as ONE launch of csrc/pointwise_wide_bf16.hip, or None where
    mlp_bf16_wide_plan refuses (the caller keeps its route).  bn in training mode enters with its batch statistics (_stats, as
    bn_act_conv), in eval mode with its running ones; bn2 enters as sparse_ops.fold_bn's (scale, shift).  ``cols`` = (c0, c1):
    the conv's weight columns c0 .. c1 - 1 applied to x's c1 - c0 channels (no copy: the kernel reads the slice in place).  An x
    that is not 8-byte aligned (only the address is looked at) is refused here too, so the entry point's MGAR_EUNSUPPORTED is
    never reached from the host."""
    cin = None if cols is None else cols[1] - cols[0]
    if not mlp_bf16_wide_plan(x, conv, bn, bn2, others, pool, cin):
        return None
    c, cout = x.shape[1], conv.out_channels
    x3 = x.contiguous().flatten(2)
    if x3.data_ptr() % 8 != 0:      # a view whose storage offset breaks the kernel's 8-byte alignment: the caller's route
        return None
    wfull = _f32(conv.weight.detach()).reshape(cout, conv.in_channels)
    wfull = wfull if wfull.is_contiguous() else wfull.contiguous()
    w = wfull if cols is None else wfull[:, cols[0]:cols[1]]
    pro = epi = None
    if bn is not None:
        mean, invstd = _stats(x3, bn, in_stats)
        gamma, beta = _affine(bn, c, x.device)
        pro = (mean, invstd, gamma.detach(), beta.detach())
    if bn2 is not None:
        from .sparse_ops import fold_bn
        epi = fold_bn(bn2)
    y = _wide_launch(x3, w, conv.in_channels, cout, pro, relu, epi, relu2, x.shape[3] if pool else 0)
    return y if pool else y.view(x.shape[0], cout, *x.shape[2:])


def bn_act_conv(x, bn, relu, conv, rowmajor_grad=False, in_stats=None, want_out_stats=False, others=(), eval_steps=True):
    """conv(relu?(bn(x))) for a bias-free kernel-size-1 ``conv`` in one fused step, or None if the
    shapes are outside the fused kernel (the caller then runs bn_act and the GEMM separately).  ``others``, ``eval_steps``: the
    further modules of the step and the caller's consent to the inference form (eval_mlp_plan)."""
    if not bn.training:   # inference: the same kernel on the running statistics (eval_mlp_plan), else the caller's route
        y = _bn_act_conv_eval(x, bn, relu, conv, others) if eval_steps else None
        return y if y is None or not want_out_stats else (y, None)
    if not (x.is_cuda and x.dtype in _PAYLOADS and bn.training and x.dim() >= 3 and conv.bias is None):
        return None
    if x.dtype != torch.float32 and _needs_grad(x, (conv.weight,)):
        return None   # the weight-gradient kernel (csrc/pointwise_dw.hip) takes fp32 payloads only: bf16 is a forward path
    c, cout = x.shape[1], conv.out_channels
    x3 = x.contiguous().flatten(2)
    if c > FUSED_CONV_MAX_CHANNELS or cout > FUSED_CONV_MAX_CHANNELS or x3.shape[2] % 4 != 0 \
            or x3.shape[0] * x3.shape[2] < (1 << 16):
        return None
    mean, invstd = _stats(x3, bn, in_stats)
    gamma, beta = _affine(bn, c, x.device)
    needs_grad = _needs_grad(x, (conv.weight, gamma, beta))
    if mlp_bf16_mfma_plan(x3, cout, needs_grad, bn):
        y = _conv_bf16_mfma(x3, _f32(conv.weight.detach()).view(cout, c), mean, invstd, gamma.detach(), beta.detach(), relu)
        y = y.view(x.shape[0], cout, *x.shape[2:])
        return (y, None) if want_out_stats else y   # bf16 has no statistics epilogue (stats_partial_buffer)
    out_stats = stats_partial_buffer(x3, cout, x3.shape[0] * x3.shape[2]) \
        if want_out_stats and cout <= FUSED_STATS_MAX_CHANNELS and x3.shape[2] % STATS_TILE == 0 else None
    y = _BnActConv.apply(x3, gamma, beta, mean, invstd, relu, _f32(conv.weight).view(cout, c), rowmajor_grad, out_stats)
    y = y.view(x.shape[0], cout, *x.shape[2:])
    return (y, out_stats) if want_out_stats else y


# Backward of the last two layers of a shared MLP without the dense gradient of the max-pool layer (_BnActConvBnMaxPool).  False
# = the two separate nodes (_BnActConv, _BnActMaxPool), which stay the route of every shape the folded kernels do not take.
FOLD_MAXPOOL_BWD = True


def bn_act_conv_maxpool(x, bn, relu, conv, bn2, relu2, rowmajor_grad=False, in_stats=None):
    """max over the last axis of relu2?(bn2(conv(relu?(bn(x))))) for x (B, C, M, ns) -> (B, Ck, M) as one autograd node whose
    backward skips the max-pool layer's dense gradient, or None outside its shapes (the caller then runs bn_act_conv and
    bn_act_maxpool): fp32, training statistics in both BatchNorms, both channel counts <= 64, ns % 4 == 0, B * M * ns >= 65 536."""
    if not (FOLD_MAXPOOL_BWD and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and torch.is_grad_enabled()
            and bn.training and bn2.training and conv.bias is None):
        return None
    b, c, m, ns = x.shape
    ck = conv.out_channels
    if c > FUSED_CONV_MAX_CHANNELS or ck > FUSED_CONV_MAX_CHANNELS or ns % 4 != 0 or ns > 255 or b * m * ns < (1 << 16):
        return None
    x3 = x.contiguous().flatten(2)
    mean, invstd = _stats(x3, bn, in_stats)
    gamma, beta = _affine(bn, c, x.device)
    gamma2, beta2 = _affine(bn2, ck, x.device)
    return _BnActConvBnMaxPool.apply(x3, gamma, beta, mean, invstd, relu, _f32(conv.weight).view(ck, c), gamma2, beta2, bn2, relu2,
                                     m, ns, rowmajor_grad)


def _affine(bn, c, device):
    if bn.affine:
        return _f32(bn.weight), _f32(bn.bias)
    return torch.ones(c, device=device), torch.zeros(c, device=device)


def _stats(x3, bn, partial=None):
    if bn.training or not bn.track_running_stats:
        return _train_stats(x3, bn, partial)
    return _f32(bn.running_mean), torch.rsqrt(_f32(bn.running_var) + bn.eps)


def _slice_stride(out, x):
    """out: a (B, C, ...) CHANNEL SLICE of a wider contiguous (B, C_total, ...) tensor (what y[:, c0:c1] is) with x's shape
    and dtype -> its batch stride in elements, or None if it is anything else."""
    if out is None or out.shape != x.shape or out.dtype != x.dtype or not out.is_cuda:
        return None
    inner = 1
    for size, stride in zip(reversed(out.shape[1:]), reversed(out.stride()[1:])):
        if size != 1 and stride != inner:
            return None
        inner *= size
    return out.stride(0) if out.stride(0) >= inner else None


# ---- channels-last (NDHWC) activations of the frozen I3D (csrc/channels_last.hpp) -------------------------------------------
def is_channels_last_3d(x):
    return x.dim() == 5 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last_3d)


def _cl_out_slice(out, x):
    """out = y[:, c0:c0 + C] of a channels-last (N, C_total, T, H, W) tensor with x's shape / dtype -> its row stride C_total."""
    if out is None or out.shape != x.shape or out.dtype != x.dtype or not out.is_cuda:
        return None
    n, c, t, h, w = out.shape
    ld = out.stride(4)
    ok = out.stride(1) == 1 and ld >= c and out.stride(3) == w * ld and out.stride(2) == h * w * ld and out.stride(0) == t * h * w * ld
    return ld if ok and ld % 4 == 0 and (out.data_ptr() // out.element_size()) % 4 == 0 else None


def _cl_stats(x, bn, per_sample):
    n, c, t, h, w = x.shape
    r = t * h * w
    rows = n * c if per_sample else c
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    ws = torch.empty((max(L.raw("mgar_bn_cl_workspace_floats", n, r, c, int(per_sample)), 1),), dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    L.payload_call("mgar_bn_cl_train_stats", x.dtype, x.data_ptr(), n, r, c, int(per_sample), float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1), L.fptr(ws), L.fptr(mean), L.fptr(invstd),
                   L.fptr(bn.running_mean) if track else None, L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
                   L.stream_of(x))
    return mean, invstd


def bn_act_channels_last(x, bn, relu, per_sample, out=None):
    """[relu](bn_train(x)) for a channels-last x (forward only; frozen I3D); ``out``: a channel slice of a wider channels-last
    tensor (the Inception concatenation).  None if the shapes do not qualify (C % 4, C > 1024, dtype)."""
    n, c, t, h, w = x.shape
    if c % 4 != 0 or c > 1024 or x.dtype not in _PAYLOADS or (per_sample and n * c > 65535) or not bn.training:
        return None
    mean, invstd = _cl_stats(x, bn, per_sample)
    gamma, beta = _affine(bn, c, x.device)
    ld = _cl_out_slice(out, x)
    y = out if ld is not None else torch.empty_like(x)           # preserve_format: channels-last
    L.payload_call("mgar_bn_cl_act_fwd", x.dtype, x.data_ptr(), n, t * h * w, c, int(per_sample), L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), y.data_ptr(), ld if ld is not None else c, L.stream_of(x))
    return y


def bn_act_to_channels_last(x, bn, relu, per_sample):
    """The same for a contiguous NCDHW x, RESULT channels-last: where the I3D's activations change layout (after the stem)."""
    x = x.contiguous()
    n, c, t, h, w = x.shape
    if x.dtype not in _PAYLOADS or not bn.training or (per_sample and n * c > 65535):
        return None
    x3 = x.flatten(2)
    if per_sample:
        mean = torch.empty((n * c,), dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        track = bn.track_running_stats and bn.running_mean is not None
        ws = _workspace(x3, 1, n * c, x3.shape[2])
        L.payload_call("mgar_bn_train_stats_grouped", x.dtype, L.pptr(x3, x.dtype), n, c, x3.shape[2], float(bn.eps),
                       float(bn.momentum if bn.momentum is not None else 0.1), L.fptr(ws), L.fptr(mean), L.fptr(invstd),
                       L.fptr(bn.running_mean) if track else None, L.fptr(bn.running_var) if track else None,
                       L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
                       L.stream_of(x))
    else:
        mean, invstd = _train_stats(x3, bn)
    gamma, beta = _affine(bn, c, x.device)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last_3d)
    L.payload_call("mgar_bn_act_fwd_to_cl", x.dtype, L.pptr(x3, x.dtype), n, c, t * h * w, int(per_sample), L.fptr(mean), L.fptr(invstd),
                   L.fptr(gamma), L.fptr(beta), int(relu), y.data_ptr(), c, L.stream_of(x))
    return y


class _BnActRows(Function):
    """y = [relu](batch_norm_train(x)) for ROW-MAJOR x (rows, C): the sparse trunk's features (csrc/channels_last.hpp)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, invstd, relu):
        rows, c = x.shape
        y = torch.empty_like(x)
        L.call("mgar_bn_cl_act_fwd", L.fptr(x), 1, rows, c, 0, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta), int(relu),
               L.fptr(y), c, L.stream_of(x))
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        rows, c = x.shape
        dy = dy.contiguous()
        dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty((L.raw("mgar_bn_rows_bwd_workspace_floats", rows, c),), dtype=torch.float32, device=x.device)
        L.call("mgar_bn_rows_bwd", L.fptr(dy), L.fptr(x), rows, c, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
               int(ctx.relu), L.fptr(ws), L.fptr(dgamma), L.fptr(dbeta), L.fptr(dx), L.stream_of(x))
        return dx, dgamma, dbeta, None, None, None


def bn_act_rows(x, bn, relu):
    """[relu](bn(x)) for a row-major (rows, C) device tensor and an nn.BatchNorm1d in TRAIN mode (batch statistics, running
    statistics updated) on the row-major kernels; None if the shapes do not qualify (C % 4, C > 1024, eval).  fp32 rows: forward +
    backward.  bf16 rows: forward only (None if a gradient is required) -- bf16 in and out, statistics and affine in fp32."""
    if not (x.is_cuda and x.dim() == 2 and x.dtype in _PAYLOADS and bn.training and x.shape[1] % 4 == 0 and x.shape[1] <= 1024
            and x.shape[0] > 0):
        return None
    dt = x.dtype
    if dt != torch.float32 and _needs_grad(x, (bn.weight,)):
        return None   # the row-major backward (mgar_bn_rows_bwd) takes fp32 payloads only
    x = x.contiguous()
    rows, c = x.shape
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    ws = torch.empty((max(L.raw("mgar_bn_cl_workspace_floats", 1, rows, c, 0), 1),), dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    L.payload_call("mgar_bn_cl_train_stats", dt, L.pptr(x, dt), 1, rows, c, 0, float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1), L.fptr(ws), L.fptr(mean), L.fptr(invstd),
                   L.fptr(bn.running_mean) if track else None, L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
                   L.stream_of(x))
    gamma, beta = _affine(bn, c, x.device)
    if dt != torch.float32:
        y = torch.empty_like(x)
        L.payload_call("mgar_bn_cl_act_fwd", dt, L.pptr(x, dt), 1, rows, c, 0, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                       int(relu), L.pptr(y, dt), c, L.stream_of(x))
        return y
    return _BnActRows.apply(x, gamma, beta, mean, invstd, relu)


SMALL_CHANNEL_MAX = 16384   # csrc/bn_act.hip, bn_small_fused_kernel: elements per channel one workgroup keeps in registers


def _small_fused(x, x3, bn, relu, per_sample, out):
    """Statistics + apply in one launch for small channels (forward only), or None if the shapes do not qualify."""
    b, c, p = x3.shape
    if (p if per_sample else b * p) > SMALL_CHANNEL_MAX or p % 4 != 0 or x3.dtype not in _PAYLOADS:
        return None
    bstride = _slice_stride(out, x)
    y = out if bstride is not None else torch.empty_like(x)
    track = bn.track_running_stats and bn.running_mean is not None
    rows = b * c if per_sample else c
    need = per_sample and track
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if need else None
    ws = torch.empty((rows,), dtype=torch.float32, device=x.device) if need else None
    gamma, beta = _affine(bn, c, x.device)
    dt = x3.dtype
    L.payload_call("mgar_bn_act_small", dt, L.pptr(x3, dt), b, c, p, int(per_sample), float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1), L.fptr(gamma), L.fptr(beta), int(relu),
                   L.fptr(ws) if ws is not None else None, L.fptr(mean) if mean is not None else None, None,
                   L.fptr(bn.running_mean) if track else None, L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None,
                   y.data_ptr(), bstride if bstride is not None else -1, L.stream_of(x3))
    return y


def _apply_into(x3, bn, relu, mean, invstd, per_sample, out, bstride):
    b, c, p = x3.shape
    gamma, beta = _affine(bn, c, x3.device)
    dt = x3.dtype
    L.payload_call("mgar_bn_act_fwd_into", dt, L.pptr(x3, dt), b, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                   int(relu), int(per_sample), out.data_ptr(), bstride, L.stream_of(x3))
    return out


def bn_act(x, bn, relu, rowmajor_grad=False, out=None, in_stats=None, to_channels_last=False):
    """[relu](bn(x)) for x (B, C, ...) contiguous on the device; ``bn`` is the nn.BatchNormNd module.
    ``out``: write the result into this channel slice of a wider tensor (forward-only callers; see _slice_stride).
    A channels-last 5-D x (forward only) stays channels-last; ``to_channels_last``: NCDHW in, channels-last out."""
    if x.is_cuda and x.dim() == 5 and not _needs_grad(x, (bn.weight,)):
        y = bn_act_channels_last(x, bn, relu, False, out) if is_channels_last_3d(x) else \
            (bn_act_to_channels_last(x, bn, relu, False) if to_channels_last else None)
        if y is not None:
            return y
    x3 = x.contiguous().flatten(2) if x.dim() > 2 else x.contiguous().unsqueeze(-1)
    if not bn.training and torch.is_grad_enabled() and x.requires_grad:
        return None  # eval-mode backward: let the caller take the plain torch path
    forward_only = not _needs_grad(x, (bn.weight,))
    if forward_only and bn.training and x.is_cuda and in_stats is None:
        y = _small_fused(x, x3, bn, relu, False, out)
        if y is not None:
            return y
    mean, invstd = _stats(x3, bn, in_stats)
    bstride = _slice_stride(out, x)
    if bstride is not None and x.dtype in _PAYLOADS and forward_only:
        return _apply_into(x3, bn, relu, mean, invstd, False, out, bstride)
    gamma, beta = _affine(bn, x3.shape[1], x.device)
    return _BnAct.apply(x3, gamma, beta, mean, invstd, relu, rowmajor_grad).view(x.shape)


def bn_act_per_sample(x, bn, relu, out=None, to_channels_last=False):
    """[relu](bn(x)) where every sample of x (G, C, ...) is normalised with its own batch statistics and the running
    statistics get the G momentum updates in sample order: G clips through a train-mode BatchNorm in ONE pass, with
    the result of feeding them one at a time.  Forward only (frozen I3D); None if that does not apply."""
    if not (x.is_cuda and x.dtype in _PAYLOADS and bn.training and x.dim() >= 3) or _needs_grad(x, (bn.weight,)):
        return None
    if x.dim() == 5:
        y = bn_act_channels_last(x, bn, relu, True, out) if is_channels_last_3d(x) else \
            (bn_act_to_channels_last(x, bn, relu, True) if to_channels_last else None)
        if y is not None:
            return y
    x3 = x.contiguous().flatten(2)
    g, c, p = x3.shape
    if g * c > 65535:
        return None
    y = _small_fused(x, x3, bn, relu, True, out)
    if y is not None:
        return y
    mean = torch.empty((g * c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    track = bn.track_running_stats and bn.running_mean is not None
    ws = _workspace(x3, 1, g * c, p)
    st = L.stream_of(x3)
    dt = x3.dtype
    L.payload_call("mgar_bn_train_stats_grouped", dt, L.pptr(x3, dt), g, c, p, float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1),
                   L.fptr(ws), L.fptr(mean), L.fptr(invstd), L.fptr(bn.running_mean) if track else None,
                   L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None, st)
    bstride = _slice_stride(out, x)
    if bstride is not None:
        return _apply_into(x3, bn, relu, mean, invstd, True, out, bstride)
    gamma, beta = _affine(bn, c, x.device)
    y = torch.empty_like(x3)
    L.payload_call("mgar_bn_act_fwd_grouped", dt, L.pptr(x3, dt), g, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                   int(relu), L.pptr(y, dt), st)
    return y.view(x.shape)


def bn_train_stats_only(x, bn, per_sample=False):
    """Batch statistics (mean, invstd) of x (G, C, ...) for a train-mode ``bn`` -- running statistics and the batch counter
    updated exactly as a forward pass does -- without applying anything; per_sample: every sample its own statistics, (G * C)
    vectors.  None where the grouped kernel does not apply."""
    x3 = x.contiguous().flatten(2)
    g, c, p = x3.shape
    if not per_sample:
        return _train_stats(x3, bn)
    if g * c > 65535:
        return None
    mean = torch.empty((g * c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    track = bn.track_running_stats and bn.running_mean is not None
    ws = _workspace(x3, 1, g * c, p)
    dt = x3.dtype
    L.payload_call("mgar_bn_train_stats_grouped", dt, L.pptr(x3, dt), g, c, p, float(bn.eps),
                   float(bn.momentum if bn.momentum is not None else 0.1),
                   L.fptr(ws), L.fptr(mean), L.fptr(invstd), L.fptr(bn.running_mean) if track else None,
                   L.fptr(bn.running_var) if track else None,
                   L.dev_ptr(bn.num_batches_tracked, torch.int64) if track and bn.num_batches_tracked is not None else None, L.stream_of(x3))
    return mean, invstd


def bn_apply_with_stats(x, bn, relu, stats, per_sample=False):
    """[relu]((x - mean) * invstd * gamma + beta) with GIVEN statistics (forward only): x may be a different tensor than the one
    the statistics were taken from (Unit3D.forward_then_pool: the pooled tensor)."""
    mean, invstd = stats
    x3 = x.contiguous().flatten(2)
    g, c, p = x3.shape
    gamma, beta = _affine(bn, c, x.device)
    y = torch.empty_like(x3)
    dt = x3.dtype
    if per_sample:
        L.payload_call("mgar_bn_act_fwd_grouped", dt, L.pptr(x3, dt), g, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                       int(relu), L.pptr(y, dt), L.stream_of(x3))
    else:
        L.payload_call("mgar_bn_act_fwd", dt, L.pptr(x3, dt), g, c, p, L.fptr(mean), L.fptr(invstd), L.fptr(gamma), L.fptr(beta),
                       int(relu), L.pptr(y, dt), L.stream_of(x3))
    return y.view(x.shape)


def bn_act_maxpool(x, bn, relu, in_stats=None):
    """max over the last axis of [relu](bn(x)) for x (B, C, M, ns) -> (B, C, M).  in_stats: statistics partials of x left by
    its producer kernel (stats_partial_buffer)."""
    x4 = x.contiguous()
    if x4.shape[-1] > 255 or (not bn.training and torch.is_grad_enabled() and x.requires_grad):
        return None
    mean, invstd = _stats(x4.flatten(2), bn, in_stats)
    gamma, beta = _affine(bn, x4.shape[1], x.device)
    return _BnActMaxPool.apply(x4, gamma, beta, mean, invstd, relu)[0]
