"""Inference route of the fusion net's tail (model/gat_model.py GAR_Fusion_Net3): one launch of csrc/scene_tail_eval.hip for
everything between the fused rows and the heads -- cosine similarity, D_embed, the diagonal, the zero-padded A_list, the
predicted group ids, the group max-pool and the cardinality feature -- instead of the chain of small torch launches of
forward_packed / _forward_batched.  The group ids (S, MNP) int32, -1 in the padding, are an output of their own.

MGAR_SCENE_TAIL_FUSE=0 (or SCENE_TAIL_FUSE, for tests) restores the torch route.  Train mode, a required gradient, the crossAtt
and bilinear adjacencies and the scene-by-scene route never leave it."""
import os
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib as L
from .eval_route import cached, hooked, needs_grad

SCENE_TAIL_FUSE = os.environ.get("MGAR_SCENE_TAIL_FUSE", "1") != "0"
MAX_HIDDEN = 8

TailPlan = namedtuple("TailPlan", "hidden linears")
TailPlan.__doc__ = """hidden: 0 for Linear(2, 1) + Sigmoid, H for Linear(2, H) + ReLU + Linear(H, 1) + Sigmoid; linears: the
nn.Linear modules of D_embed in order."""


def _embed_parts(d_embed):
    """TailPlan of a D_embed built as GAR_Fusion_Net3 builds it for the cosine adjacency, else None."""
    if not isinstance(d_embed, nn.Sequential):
        return None
    mods = list(d_embed)
    if len(mods) == 2 and isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.Sigmoid):
        lin = mods[0]
        if (lin.in_features, lin.out_features) == (2, 1) and lin.bias is not None:
            return TailPlan(0, (lin,))
        return None
    if (len(mods) == 4 and isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.ReLU) and isinstance(mods[2], nn.Linear)
            and isinstance(mods[3], nn.Sigmoid)):
        l1, l2 = mods[0], mods[2]
        h = l1.out_features
        if (l1.in_features == 2 and 1 <= h <= MAX_HIDDEN and (l2.in_features, l2.out_features) == (h, 1)
                and l1.bias is not None and l2.bias is not None):
            return TailPlan(h, (l1, l2))
    return None


def scene_tail_refusal(net, fused, counts=None):
    """Why a forward of the fusion net `net` on the fused rows does NOT take the fused tail -- a short reason -- or None when it
    does.  Reads nothing but attributes and host ints: no device work, no synchronisation."""
    from .model.gat_model import _BILINEAR_ADJACENCY
    if not SCENE_TAIL_FUSE:
        return "switch off"
    if net.training:
        return "training"
    d_embed = getattr(net, "D_embed", None)
    if net.cfg.FUSION == "crossAtt" or net.cfg.FUSION in _BILINEAR_ADJACENCY:
        return "adjacency"
    if not net._scene_counts_ok([2] if counts is None else list(counts)):
        return "configuration"
    parts = _embed_parts(d_embed)
    if parts is None:
        return "structure"
    if not torch.is_tensor(fused) or fused.dim() != 2 or fused.dtype != torch.float32:
        return "payload"
    if needs_grad(fused, d_embed.parameters()):
        return "gradient"
    if hooked(d_embed, *d_embed):
        return "hook"
    if fused.shape[1] % 64 != 0:
        return "size"
    if not fused.is_cuda or any(p.device != fused.device for p in d_embed.parameters()):
        return "device"
    return None


def scene_tail_plan(net, fused, counts=None):
    """The fused tail of `net` on the fused rows -- a TailPlan -- or None for the torch route.  Fused when the switch is on, the
    net is in eval mode, nothing needs a gradient (grad mode off, or neither the rows nor a parameter of D_embed requires one),
    no forward hook sits on D_embed, the adjacency is the cosine / D_embed one (not crossAtt, not the bilinear ones), the
    configuration and the counts pass _scene_counts_ok, and the rows are fp32 on the device with D % 64 == 0."""
    return _embed_parts(net.D_embed) if scene_tail_refusal(net, fused, counts) is None else None


def embed_params(d_embed, plan=None):
    """The parameter block the kernel reads, fp32 on the parameters' device: [w_v, w_g, b] for hidden == 0, else W1 (H, 2)
    row-major, b1 (H), w2 (H), b2.  Device ops only; cached on the module (eval_route.cached) under every tensor read: a frozen
    model builds it once, an in-place update of any tensor rebuilds it."""
    plan = plan or _embed_parts(d_embed)
    if plan is None:
        raise L.MgarError("scene_tail_eval: D_embed is not Linear(2,1)+Sigmoid or Linear(2,H<=8)+ReLU+Linear(H,1)+Sigmoid")
    read = [t for lin in plan.linears for t in (lin.weight, lin.bias)]
    return cached(d_embed, "_mgar_tail_params", read,
                  lambda: torch.cat([t.detach().float().reshape(-1) for t in read]).contiguous())


def scene_tail_eval_fwd(fused, dg, scene_off, de_off, counts, mnp, params, hidden):
    """The C entry point on device tensors: counts are the host ints the offsets were built from -> (A_list (S, mnp, mnp),
    group_id (S, mnp) int32, sg_features (rows, D), card_feature (S, D + 1)).  Scene sizes outside 2..MGAR_DAFM_MAX_N, a scene
    wider than mnp, D % 64 != 0 and hidden > 8 are refused by the library before anything is launched."""
    if not fused.is_cuda:
        raise L.MgarError("expected a device (HIP) tensor, got %s -- there is no CPU path" % fused.device)
    counts = [int(c) for c in counts]
    s, (rows, d) = len(counts), fused.shape
    if rows != sum(counts) or dg.numel() != sum(c * c for c in counts):
        raise L.MgarError("scene_tail_eval: %d rows / %d pairs do not match the counts" % (rows, dg.numel()))
    if params.numel() != (3 if hidden == 0 else 4 * hidden + 1):
        raise L.MgarError("scene_tail_eval: parameter block of %d floats does not match hidden = %d" % (params.numel(), hidden))
    a_list = torch.empty((s, mnp, mnp), device=fused.device, dtype=torch.float32)
    group_id = torch.empty((s, mnp), device=fused.device, dtype=torch.int32)
    sg = torch.empty_like(fused)
    card = torch.empty((s, d + 1), device=fused.device, dtype=torch.float32)
    L.call("mgar_scene_tail_eval_fwd", s, rows, d, int(mnp), min(counts) if counts else 0, max(counts) if counts else 0,
           L.iptr(scene_off), L.iptr(de_off), L.fptr(fused), L.fptr(dg), L.fptr(params), int(hidden), L.fptr(a_list),
           L.iptr(group_id), L.fptr(sg), L.fptr(card), L.stream_of(fused))
    return a_list, group_id, sg, card


def scene_tail_eval(fused, dg, layout, d_embed):
    """fused (rows, D) fp32 packed scene rows, dg the packed GIoU pairs of scene_pair_geometry, layout = scene_layout(counts,
    mnp, device), d_embed the fusion net's D_embed -> (A_list, group_id, sg_features, card_feature); no gradient."""
    plan = _embed_parts(d_embed)
    params = embed_params(d_embed, plan)
    return scene_tail_eval_fwd(fused.detach().contiguous(), dg.detach().contiguous(), layout.scene_off, layout.de_off,
                               layout.counts, layout.mnp, params, plan.hidden)


# ---------------------------------------------------------------------------------------------- eval-mode parameter caches
def stacked_head_params(net, prefix, heads, ks):
    """(w1, b1, block-diagonal w2, b2) of the seven heads that share a feature, as _heads_stacked builds them on every call,
    cached (eval_route.cached) in the net's per-prefix store under every tensor read: a frozen model builds them once.
    Built by the same ops in the same order, so the values are the bits _heads_stacked computes itself."""
    read = [t for h in heads for t in (h[0].weight, h[0].bias, h[3].weight, h[3].bias)]

    def build():
        hid_dim = heads[0][0].out_features
        w1 = torch.cat([h[0].weight for h in heads], 0)
        b1 = torch.cat([h[0].bias for h in heads], 0)
        w2 = w1.new_zeros(sum(ks), len(heads) * hid_dim)
        row = 0
        for i, (h, k) in enumerate(zip(heads, ks)):
            w2[row:row + k, i * hid_dim:(i + 1) * hid_dim] = h[3].weight
            row += k
        return w1, b1, w2, torch.cat([h[3].bias for h in heads], 0)
    return cached(net.__dict__.setdefault("_mgar_stacked_heads", {}), prefix, read, build)


def eval_bn(bn, x):
    """Eval-mode BatchNorm1d of the fused route: one addcmul on the (scale, shift) pair sparse_ops.fold_bn caches."""
    from .sparse_ops import fold_bn
    scale, shift = fold_bn(bn)
    return torch.addcmul(shift, x, scale)
