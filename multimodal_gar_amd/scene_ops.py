"""Per-scene operations on packed scene rows (HIP, csrc/scene_ops.hip): scene BatchNorm, pair geometry (De, Dg) and the
Gram matrix -- what the fusion net's batched route needs when the scenes of a batch hold different numbers of actors.
Rows of all scenes are stacked; scene_layout() builds, once per count tuple, the offsets and index tensors that carry
packed rows and packed (n_s, n_s) blocks into the zero-padded (S, MNP, ...) tensors of the reference interface."""
from collections import namedtuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L
from .dafm_ops import scene_offsets

SceneLayout = namedtuple("SceneLayout", "counts rows pairs n_max scene_off de_off row_scene row_slot pair_index diag_index "
                                        "row_local mnp")
SceneLayout.__doc__ = """counts: host tuple; rows = sum n_s; pairs = sum n_s^2; scene_off (S+1) / de_off (S) int32 as for
dafm_attention; row_scene (rows): scene id of every packed row; row_slot (rows): s * MNP + i, the row's place in a padded
(S, MNP, .) tensor viewed as (S * MNP, .); pair_index (pairs): (s * MNP + i) * MNP + j, the place of every packed pair in
(S, MNP, MNP) viewed flat; diag_index (rows): position of every (i, i) in the packed pairs; row_local (rows): s * n_max + i,
the row's place in a (S, n_max, .) tensor; mnp: the padded slots per scene the indices were built for."""

_LAYOUT_CACHE = {}


def scene_layout(counts, mnp, device):
    """Built on the host from the count list and cached per (counts, mnp, device): after the first call with a given
    count tuple nothing here touches the host.  Scenes above MGAR_DAFM_MAX_N actors raise (dafm_ops.scene_offsets)."""
    counts = tuple(int(c) for c in counts)
    key = (counts, int(mnp), str(device))
    hit = _LAYOUT_CACHE.get(key)
    if hit is not None:
        return hit
    if any(c > mnp for c in counts):
        raise ValueError("scene_layout: a scene of %d actors does not fit %d padded slots" % (max(counts), mnp))
    so, do = scene_offsets(counts, device)          # raises on n_s outside 0..MGAR_DAFM_MAX_N
    n_max = max(counts) if counts else 0
    row_scene, row_slot, row_local, pair_index, diag_index = [], [], [], [], []
    m = 0
    for s, n in enumerate(counts):
        i = torch.arange(n, dtype=torch.int64)
        row_scene.append(torch.full((n,), s, dtype=torch.int64))
        row_slot.append(s * mnp + i)
        row_local.append(s * n_max + i)
        pair_index.append((((s * mnp + i) * mnp)[:, None] + i[None, :]).reshape(-1))
        diag_index.append(m + i * (n + 1))
        m += n * n

    def dev(parts):
        return (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)).to(device)

    out = SceneLayout(counts, sum(counts), m, n_max, so, do, dev(row_scene), dev(row_slot), dev(pair_index), dev(diag_index),
                      dev(row_local), int(mnp))
    if len(_LAYOUT_CACHE) < 64:
        _LAYOUT_CACHE[key] = out
    return out


class _SceneBatchNorm(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, scene_off, running_mean, running_var, num_batches_tracked, eps, momentum):
        x = x.contiguous()
        rows, c = x.shape
        n_scenes = scene_off.numel() - 1
        y = torch.empty_like(x)
        mean, invstd, var = (torch.empty((n_scenes, c), device=x.device, dtype=x.dtype) for _ in range(3))
        nbt = None if num_batches_tracked is None else L.dev_ptr(num_batches_tracked, torch.int64)
        L.call("mgar_scene_bn_fwd", n_scenes, rows, c, L.iptr(scene_off), L.fptr(x), L.fptr(weight), L.fptr(bias), float(eps),
               float(momentum), L.fptr(running_mean), L.fptr(running_var), nbt, L.fptr(y), L.fptr(mean), L.fptr(invstd),
               L.fptr(var), L.stream_of(x))
        ctx.save_for_backward(x, weight, scene_off, mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight, scene_off, mean, invstd = ctx.saved_tensors
        rows, c = x.shape
        n_scenes = scene_off.numel() - 1
        grad_y = grad_y.contiguous()
        gx = torch.empty_like(x)
        if n_scenes == 0 or rows == 0:
            return gx, torch.zeros_like(weight), torch.zeros_like(weight), None, None, None, None, None, None
        gw, gb = torch.empty_like(weight), torch.empty_like(weight)
        work = torch.empty((2, n_scenes, c), device=x.device, dtype=x.dtype)
        L.call("mgar_scene_bn_bwd", n_scenes, rows, c, L.iptr(scene_off), L.fptr(x), L.fptr(grad_y), L.fptr(weight), L.fptr(mean),
               L.fptr(invstd), L.fptr(work), L.fptr(gx), L.fptr(gw), L.fptr(gb), L.stream_of(x))
        return gx, gw, gb, None, None, None, None, None, None


def scene_batch_norm(x, weight, bias, scene_off, running_mean=None, running_var=None, num_batches_tracked=None, eps=1e-5,
                     momentum=0.1):
    """Training-mode BatchNorm1d of every scene by itself over packed x (rows, C), C % 64 == 0.  The running statistics,
    when given, are updated in place: one EMA step per scene of at least two rows, in scene order."""
    return _SceneBatchNorm.apply(x.float(), weight.float(), bias.float(), scene_off, running_mean, running_var,
                                 num_batches_tracked, eps, momentum)


def scene_pair_geometry(centres, boxes, scene_off, de_off, pairs):
    """centres (rows, 3), boxes (rows, 4) xyxy or None -> (De, Dg) packed like dafm_attention's de_flat (`pairs` floats each;
    Dg is None without boxes).  No gradient: boxes carry none."""
    centres = centres.detach().float().contiguous()
    rows = centres.shape[0]
    de = torch.empty(pairs, device=centres.device, dtype=torch.float32)
    dg = None
    if boxes is not None:
        boxes = boxes.detach().float().contiguous()
        dg = torch.empty_like(de)
    L.call("mgar_scene_pair_geometry", scene_off.numel() - 1, rows, L.iptr(scene_off), L.iptr(de_off), L.fptr(centres),
           L.fptr(boxes), L.fptr(de), L.fptr(dg), L.stream_of(centres))
    return de, dg


class _SceneGram(Function):
    @staticmethod
    def forward(ctx, x, scene_off, de_off, pairs):
        x = x.contiguous()
        rows, d = x.shape
        g = torch.empty(pairs, device=x.device, dtype=x.dtype)
        L.call("mgar_scene_gram_fwd", scene_off.numel() - 1, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(x), L.fptr(g),
               L.stream_of(x))
        ctx.save_for_backward(x, scene_off, de_off)
        return g

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_g):
        x, scene_off, de_off = ctx.saved_tensors
        rows, d = x.shape
        gx = torch.empty_like(x)
        L.call("mgar_scene_gram_bwd", scene_off.numel() - 1, rows, d, L.iptr(scene_off), L.iptr(de_off), L.fptr(x),
               L.fptr(grad_g.contiguous()), L.fptr(gx), L.stream_of(x))
        return gx, None, None, None


def scene_gram(x, scene_off, de_off, pairs):
    """x (rows, D), D % 64 == 0 -> every scene's x_s x_s^T, packed (`pairs` floats)."""
    return _SceneGram.apply(x.float(), scene_off, de_off, pairs)
