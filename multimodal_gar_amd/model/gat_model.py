"""MGAR-net model assembly on the MI355X operator set.

Mirror of the public surface of the reference's model/gat_model.py: the same class names,
constructor / forward signatures, sub-module and parameter names and shapes (so reference
checkpoints load), for
  cross_attention_fusion (:15-41), SpaTemp_self_att (:43-75),
  FusionAttention / 2 / 3 / _gaussian / _mat / _MMCA_sty / _cat / _sum / _pe (:77-865),
  LiDAR_Backbone (:868-971), RGB_Backbone (:973-1095), Actionhead (:1099-1128),
  GAR_Fusion_Net3 (:1130-1699), GAR_Fusion_ALL (:1805-1853).
GARNet / GARNet_All (:1701-1803, :1856-1949) are legacy experiments that depend on modules
missing from the reference repo (``config``, ``model.jrdb_act_rep``); they are exported as
stubs that raise on construction.

What runs where:
  * RoIAlign, DAFM attention core, GATv2 edge-softmax/aggregate, and every pointnet2 op under
    the LiDAR branch are HIP kernels behind the C ABI (include/mgar_ops.h);
  * convolutions / Linear / LayerNorm / BatchNorm are library GEMM-shaped work on PyTorch-ROCm.
``GAR_Fusion_Net3.forward`` keeps the reference's per-scene semantics exactly; when every scene
of the batch has the same number of actors and the configuration is the shipped one
(Multimodal_cfg/mil3.yaml: FUSION Attention_mat, cosine similarity, EUCLIDEAN) it takes a
batched route that evaluates all scenes in one pass -- same arithmetic, no Python loop, no
host synchronisation -- and is tested against the per-scene route.  The packed form of that
route (forward_packed: any actor counts) also serves the FUSION values of _PACKED_FUSIONS.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .backbone import *  # noqa: F401,F403  (the reference re-exports backbone through gat_model)
from .backbone import InceptionI3d, NLBlockND
from .. import vision_ops as TO
from .. import graph_ops as pyg_nn
from ..eval_route import cached
from ..metric_ops import pairwise_cosine_similarity, pairwise_euclidean_distance
from ..nonlocal_ops import nl_eval_plan
from ..dafm_ops import dafm_attention, dafm_attention_add, packed_pairs, scene_offsets
from ..scene_mha_ops import scene_multihead_attention
from ..scene_ops import scene_batch_norm, scene_gram, scene_layout, scene_pair_geometry
from .. import scene_tail_ops
from ..pcdet.models import build_network, load_data_to_gpu


def _ffn(dim):
    return nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim))


def _kaiming_param(rows, cols):
    p = nn.Parameter(torch.zeros([rows, cols]))
    torch.nn.init.kaiming_normal_(p)
    return p


class cross_attention_fusion(nn.Module):
    def __init__(self, input_dim=512, out_dim=512):
        super().__init__()
        self.Att1 = nn.MultiheadAttention(512, 8)
        self.Att2 = nn.MultiheadAttention(512, 8)
        self.LN_r_1 = nn.LayerNorm([out_dim]); self.FFN_r = _ffn(out_dim); self.LN_r_2 = nn.LayerNorm([out_dim])
        self.LN_l_1 = nn.LayerNorm([out_dim]); self.FFN_l = _ffn(out_dim); self.LN_l_2 = nn.LayerNorm([out_dim])

    def forward(self, R, L):
        # the reference uses Att1 and FFN_r for BOTH branches (:30-38); kept
        R = self.LN_r_1(self.Att1(L, R, R)[0] + R)
        R = self.LN_r_2(self.FFN_r(R) + R)
        L = self.LN_l_1(self.Att1(R, L, L)[0] + L)
        L = self.LN_l_2(self.FFN_r(L) + L)
        return torch.max(torch.stack((R, L)), dim=0)[0]

    def forward_stacked(self, R, L, scene_off, de_off, pairs):
        """`forward` for the rows of all scenes at once: R, L (sum_s n_s, 512); pairs = sum_s n_s^2 (host int).  The
        reference's conventions are kept: Att1 and FFN_r serve both branches, the L branch queries with the UPDATED R, and
        Att2 / FFN_l are never evaluated (no gradient).  The attention core is the HIP kernel of csrc/scene_mha.hip."""
        def att(query, memory):
            return scene_multihead_attention(self.Att1, query, memory, memory, scene_off, de_off, pairs)
        R = self.LN_r_1(att(L, R) + R)
        R = self.LN_r_2(self.FFN_r(R) + R)
        L = self.LN_l_1(att(R, L) + L)
        L = self.LN_l_2(self.FFN_r(L) + L)
        return torch.max(R, L)


class SpaTemp_self_att(nn.Module):
    def __init__(self, in_channels, inter_channels=None, mode='dot', pool="avg"):
        super().__init__()
        self.Spa_block = NLBlockND(in_channels, inter_channels, mode, dimension=2)
        if pool == 'flat':
            self.temp_block = NLBlockND(96 * 6 * 6, 432, mode, dimension=1)
        else:
            self.temp_block = NLBlockND(in_channels, inter_channels, mode, dimension=1)
        if pool == 'avg':
            self.pool_layer = nn.AdaptiveAvgPool2d((1))
        elif pool == 'flat':
            self.pool_layer = nn.Flatten()

    def forward(self, x):
        x = self.pool_layer(self.Spa_block(x)).squeeze()      # (N, C)
        x = x.unsqueeze(0).permute(0, 2, 1)                   # (1, C, N)
        return self.temp_block(x).permute(2, 1, 0).squeeze()  # (N, C)


# ---------------------------------------------------------------------------------------
# Two-branch cross attention R <- L and L <- R with a distance prior on the logits.
# The nine reference variants differ only in the prior and in how (R', L') are combined.
# ---------------------------------------------------------------------------------------
class _TwoBranchFusion(nn.Module):
    q_extra = 0  # extra input columns of WQ / WK (positional variant)

    def __init__(self, input_dim=512, out_dim=512, sigma=10):
        super().__init__()
        self.input_dim, self.out_dim, self.sigma = input_dim, out_dim, sigma
        for br in ("r", "l"):
            setattr(self, "WQ_" + br, _kaiming_param(input_dim + self.q_extra, out_dim))
            setattr(self, "WK_" + br, _kaiming_param(input_dim + self.q_extra, out_dim))
            setattr(self, "WV_" + br, _kaiming_param(input_dim, out_dim))
            setattr(self, "LN_%s_1" % br, nn.LayerNorm([out_dim]))
            setattr(self, "FFN_" + br, _ffn(out_dim))
            setattr(self, "LN_%s_2" % br, nn.LayerNorm([out_dim]))

    # priors: return (kind, matrix) with kind in {None, 'add', 'mul'}
    def prior_r(self, Dg, De):
        return None, None

    def prior_l(self, Dg, De, E_r):
        return None, None

    def _post(self, br, att_out, skip):
        x = getattr(self, "LN_%s_1" % br)(att_out + skip)
        x = x + getattr(self, "FFN_" + br)(x)
        return getattr(self, "LN_%s_2" % br)(x)

    def _attend(self, q, k, v, kind, prior):
        logits = torch.matmul(q, k.T)
        if kind == 'mul':
            logits = logits * prior / self.out_dim ** 0.5
        else:
            logits = logits / self.out_dim ** 0.5
            if kind == 'add':
                logits = logits + prior
        return torch.matmul(torch.softmax(logits, dim=1), v)

    def branches(self, R, L, Dg, De, Rq=None, Lq=None):
        Rq = R if Rq is None else Rq
        Lq = L if Lq is None else Lq
        kind_r, E_r = self.prior_r(Dg, De)
        R_prime = self._post("r", self._attend(Lq @ self.WQ_r, Rq @ self.WK_r, R @ self.WV_r, kind_r, E_r), R)
        kind_l, E_l = self.prior_l(Dg, De, E_r)
        L_prime = self._post("l", self._attend(Rq @ self.WQ_l, Lq @ self.WK_l, L @ self.WV_l, kind_l, E_l), L)
        return R_prime, L_prime

    def forward(self, R, L, Dg, De):
        return self.branches(R, L, Dg, De)

    def forward_stacked(self, R, L, de_flat, dg_flat, scene_off, de_off, pairs=None):
        """`branches` for the rows of all scenes at once: R, L (sum_s n_s, D); de_flat, dg_flat: the scenes' (n_s, n_s)
        matrices flattened and concatenated (None where the variant reads neither).  The priors are element-wise, so the
        per-scene formulas apply to the flat tensors as they are; the attention core is the fused HIP kernel with an
        additive prior (csrc/dafm.hip).  pairs: sum_s n_s^2 as a host int (scene_layout().pairs); without it the offsets are
        read back from the device (dafm_attention_add).  -> (R', L').
        NOTE: FusionAttention_mat.forward_stacked, which is older, takes (R, L, de_flat, scene_off, de_off) -- no dg_flat;
        GAR_Fusion_Net3._fuse_packed is the one caller and tells them apart by cfg.FUSION.  This method serves the variants
        routed there (FusionAttention, FusionAttention2 / 3, FusionAttention_gaussian); FusionAttention_cat / _sum inherit
        it and get the plain pair (R', L'), not their own combination, and the positional variant is refused below."""
        if self.q_extra:
            raise NotImplementedError("%s: no stacked route (its queries and keys take extra columns)" % type(self).__name__)
        scale = 1.0 / self.out_dim ** 0.5
        kind_r, E_r = self.prior_r(dg_flat, de_flat)
        kind_l, E_l = self.prior_l(dg_flat, de_flat, E_r)
        if 'mul' in (kind_r, kind_l):
            raise NotImplementedError("%s: no stacked route for a multiplicative prior" % type(self).__name__)
        att_r, _ = dafm_attention_add(L @ self.WQ_r, R @ self.WK_r, R @ self.WV_r, E_r, scene_off, de_off, scale, pairs)
        R_prime = self._post("r", att_r, R)
        att_l, _ = dafm_attention_add(R @ self.WQ_l, L @ self.WK_l, L @ self.WV_l, E_l, scene_off, de_off, scale, pairs)
        L_prime = self._post("l", att_l, L)
        return R_prime, L_prime


class FusionAttention(_TwoBranchFusion):
    """Plain cross attention, no prior (reference :77-156)."""


class FusionAttention3(_TwoBranchFusion):
    """R branch + exp(-De^2 / 2 sigma^2), L branch + GIoU (reference :255-339)."""

    def prior_r(self, Dg, De):
        return 'add', torch.exp(-1 / (2 * self.sigma ** 2) * (De ** 2))

    def prior_l(self, Dg, De, E_r):
        return 'add', Dg


class FusionAttention2(FusionAttention3):
    """FusionAttention3 followed by an element-wise max of the two branches (:159-252)."""

    def forward(self, R, L, Dg, De):
        Rp, Lp = self.branches(R, L, Dg, De)
        return torch.max(torch.stack((Rp, Lp)), dim=0)[0]

    def forward_stacked(self, R, L, de_flat, dg_flat, scene_off, de_off, pairs=None):
        return torch.max(*super().forward_stacked(R, L, de_flat, dg_flat, scene_off, de_off, pairs))


class FusionAttention_cat(FusionAttention3):
    def forward(self, R, L, Dg, De):
        return torch.concat(self.branches(R, L, Dg, De), dim=1)


class FusionAttention_gaussian(_TwoBranchFusion):
    """Gaussian pdf of De added to BOTH branches (the L branch reuses E_r, :413)."""

    def prior_r(self, Dg, De):
        return 'add', 1 / (self.sigma * math.sqrt(2 * math.pi)) * torch.exp((-1 / 2) * (De / self.sigma) ** 2)

    def prior_l(self, Dg, De, E_r):
        return 'add', E_r


class FusionAttention_sum(_TwoBranchFusion):
    def prior_r(self, Dg, De):
        return 'add', torch.exp(-1 / (2 * self.sigma ** 2) * (De ** 2))

    def prior_l(self, Dg, De, E_r):
        return 'add', E_r

    def forward(self, R, L, Dg, De):
        Rp, Lp = self.branches(R, L, Dg, De)
        return (Rp + Lp) / 2


class FusionAttention_pe(_TwoBranchFusion):
    q_extra = 2

    def forward(self, R, L, bb):
        return self.branches(R, L, None, None, Rq=torch.concat([bb, R], dim=1), Lq=torch.concat([bb, L], dim=1))


class FusionAttention_mat(_TwoBranchFusion):
    """The Distance-Aware Fusion Module layer the shipped config selects (mil3.yaml:147;
    reference :427-511):  E = softmax(-De/sigma, 1) multiplies the logits of BOTH branches
    (Dg is accepted and ignored, :501-503).  The attention core runs in the fused HIP kernel
    (csrc/dafm.hip), batched over scenes by ``forward_stacked``."""

    def forward(self, R, L, Dg, De):
        n = R.shape[0]
        so, do = scene_offsets([n], R.device)
        return self.forward_stacked(R, L, De.reshape(-1), so, do)

    def forward_stacked(self, R, L, de_flat, scene_off, de_off):
        """R, L: (sum_s n_s, D) rows of all scenes; de_flat: their (n_s, n_s) matrices, flattened."""
        scale = 1.0 / self.out_dim ** 0.5
        de_flat = de_flat.contiguous().float()
        att_r, _ = dafm_attention(L @ self.WQ_r, R @ self.WK_r, R @ self.WV_r, de_flat, scene_off, de_off, self.sigma, scale)
        R_prime = self._post("r", att_r, R)
        att_l, _ = dafm_attention(R @ self.WQ_l, L @ self.WK_l, L @ self.WV_l, de_flat, scene_off, de_off, self.sigma, scale)
        L_prime = self._post("l", att_l, L)
        return R_prime, L_prime


class FusionAttention_MMCA_sty(nn.Module):
    def __init__(self, input_dim=512, out_dim=512, sigma=10):
        super().__init__()
        self.input_dim, self.out_dim, self.sigma = input_dim, out_dim, sigma
        self.WQ = _kaiming_param(input_dim, out_dim)
        self.WK = _kaiming_param(input_dim, out_dim)
        self.WV = _kaiming_param(input_dim, out_dim)
        self.LN_1 = nn.LayerNorm([out_dim]); self.FFN = _ffn(out_dim); self.LN_2 = nn.LayerNorm([out_dim])

    def forward(self, R, L, Dg, De, Distance=False):
        Fcat = torch.concat([R, L], dim=0)
        Q, K, V = Fcat @ self.WQ, Fcat @ self.WK, Fcat @ self.WV
        logits = torch.matmul(Q, K.T) / self.out_dim ** 0.5
        if Distance:
            logits = logits * torch.sigmoid(torch.exp(-(De / self.sigma) ** 2)).repeat([2, 2])
        x = self.LN_1(torch.matmul(torch.softmax(logits, dim=1), V) + Fcat)
        x = self.LN_2(x + self.FFN(x))
        return x[:R.shape[0], :], x[R.shape[0]:, :]


# ---------------------------------------------------------------------------------------
class LiDAR_Backbone(nn.Module):
    """pcdet detector -> pooled per-actor features (NP, 216, 96) -> non-local block -> Linear."""

    def __init__(self, cfg, dataset):
        super().__init__()
        self.cfg = cfg
        lc = cfg.LiDAR_BACKBONE
        self.model = build_network(model_cfg=lc.MODEL, num_class=len(lc.CLASS_NAMES), dataset=dataset)
        if lc.SELF_ATT1.USE:
            self.self_attention_net1 = NLBlockND(96, inter_channels=96 // 8, mode='dot', dimension=lc.SELF_ATT1.DIM)
            self.embedding = nn.Linear(96 * 6 * 6 * (1 if lc.SELF_ATT1.INTER_PERSON else 6), 512)
        if lc.two_stage_att and lc.get('pool') == 'flat':
            self.self_attetion = SpaTemp_self_att(96, 96 // 8, mode='dot', pool='flat')
            self.embedding = nn.Linear(96 * 6 * 6, 512)
        elif lc.two_stage_att:
            self.self_attetion = SpaTemp_self_att(96, 96 // 8, mode='dot')
            self.embedding = nn.Linear(96, 512)

    def LiDAR_feature_processing(self, data_dict):
        shared = data_dict['shared_feature']
        return shared.reshape([data_dict['batch_size'], -1, shared.shape[1]])

    @staticmethod
    def _as_grid(pooled):
        n_person, _, chans = pooled.shape
        return pooled.permute(0, 2, 1).reshape(n_person, chans, 6, 6, 6)

    def forward(self, data_dict):
        out = self.model(data_dict)
        lc = self.cfg.LiDAR_BACKBONE
        if lc.two_stage_att:
            grid = F.adaptive_avg_pool3d(self._as_grid(out['pooled_features']), (6, 6, 1)).squeeze(-1)
            return self.embedding(self.self_attetion(grid).unsqueeze(0))
        if not lc.SELF_ATT1.USE:
            return self.LiDAR_feature_processing(out)
        assert lc.SELF_ATT1.DIM == 3
        nl = self.self_attention_net1
        if not (lc.SELF_ATT1.INTER_PERSON or nl._forward_hooks or nl._forward_pre_hooks) \
                and nl_eval_plan(nl, out['pooled_features'], rows=True) is not None:
            grid = nl.forward_rows(out['pooled_features'])   # inference: the (NP, 216, 96) rows as they are (a hook wants __call__)
            return self.embedding(grid.reshape(1, grid.shape[0], -1))
        grid = self._as_grid(out['pooled_features'])                         # (NP, 96, 6, 6, 6)
        if not lc.SELF_ATT1.INTER_PERSON:
            grid = self.self_attention_net1(grid)
            return self.embedding(grid.reshape(1, grid.shape[0], -1))        # (1, NP, 512)
        grid = F.adaptive_avg_pool3d(grid, (6, 6, 1)).squeeze(-1).unsqueeze(0).permute(0, 2, 1, 3, 4)
        grid = self.self_attention_net1(grid).permute(0, 2, 1, 3, 4)
        return self.embedding(grid.reshape(1, grid.shape[1], -1))


class RGB_Backbone(nn.Module):
    """I3D -> centre temporal slice -> RoIAlign 5x5 per actor -> non-local block -> avg pool ->
    Linear(832, 512) -> optional GATv2 over the fully connected actor graph.

    The reference unconditionally torch.load()s a Kinetics checkpoint from an absolute /mnt path
    (:990-991); here the path comes from ``cfg.I3D_PRETRAINED`` (optional) and is loaded with
    strict=False only if the file exists."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.backbone_net = InceptionI3d(final_endpoint='Mixed_4f')
        self.backbone_net.build()
        ckpt = cfg.get('I3D_PRETRAINED') if hasattr(cfg, 'get') else None
        if ckpt and os.path.exists(ckpt):
            self.backbone_net.load_state_dict(torch.load(ckpt, map_location='cpu'), strict=False)
        if cfg.I3D_FREEZE:
            for para in self.backbone_net.parameters():
                para.requires_grad = False
        in_channels = 832
        if cfg.two_stage_att:
            self.self_attention_net = SpaTemp_self_att(in_channels, inter_channels=in_channels // 8, mode='dot')
        else:
            self.self_attention_net = NLBlockND(in_channels, inter_channels=in_channels // 8, mode='dot',
                                                dimension=3 if cfg.INTER_PERSON else 2)
        self.pool_layer = nn.AdaptiveAvgPool2d((1))
        self.embedding_layer = nn.Linear(in_channels, cfg.EMBEDDING_DIM)
        self.GAT_module = pyg_nn.GATv2Conv(cfg.EMBEDDING_DIM, cfg.EMBEDDING_DIM, 8, dropout=0.5, concat=False)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def crop_features(self, images_in, boxes_in):
        """(B, 3, T, H, W) -> RoIAligned (sum_b len(boxes_in[b]), 832, 5, 5)."""
        feats = self.backbone_net.extract_features(images_in)
        feats = feats[:, :, feats.shape[2] // 2, :, :]
        return TO.roi_align(feats, boxes_in, output_size=5, spatial_scale=feats.shape[-1] / images_in.shape[-1])

    def embed(self, boxes_features):
        """(N, 832, 5, 5) -> (N, EMBEDDING_DIM), non INTER_PERSON route."""
        if self.cfg.two_stage_att:
            x = self.self_attention_net(boxes_features)
        else:
            x = self.pool_layer(self.self_attention_net(boxes_features))
        return self.embedding_layer(x.squeeze())

    def forward(self, images_in, boxes_in, person_id):
        _B = person_id.shape[0]
        person_num = [len(torch.unique(person_id[i])) - 1 for i in range(_B)]
        boxes_features = self.crop_features(images_in, boxes_in)
        boxes_features = boxes_features[:person_num[0]]  # only batch element 0 survives (:1059)
        if self.cfg.INTER_PERSON and not self.cfg.two_stage_att:
            x = boxes_features.unsqueeze(0).permute(0, 2, 1, 3, 4)
            x = self.pool_layer(self.self_attention_net(x))
            x = x.squeeze().reshape(_B, x.shape[1], person_num[0]).permute(0, 2, 1)
            boxes_features = self.embedding_layer(x.squeeze())
        else:
            boxes_features = self.embed(boxes_features)
        if self.cfg.GAT_module:
            boxes_len = [int((box.sum(dim=1) != 0).sum().item()) for box in boxes_in]
            boxes_features = self.GAT_module(boxes_features, fully_connected_edges(boxes_len, boxes_features.device))
        return boxes_features


_EDGE_CACHE = {}


def fully_connected_edges(boxes_len, device):
    """All ordered pairs i != j inside each scene (combinations + flip, reference :1085-1092).  The result only
    depends on the scene sizes, so it is built once per (sizes, device) and reused (no host->device copy per call;
    graph_ops caches its CSR form on the tensor)."""
    key = (tuple(int(n) for n in boxes_len), str(device))
    edges = _EDGE_CACHE.get(key)
    if edges is None:
        per_scene = [torch.combinations(torch.arange(0, n) + sum(boxes_len[:max(0, i)]), r=2) for i, n in enumerate(boxes_len)]
        pairs = torch.cat(per_scene, 0)
        edges = torch.cat((pairs, torch.flip(pairs, [1])), 0).T.contiguous().to(device)
        if len(_EDGE_CACHE) < 64:
            _EDGE_CACHE[key] = edges
    return edges


def _head(in_dim, out_dim, final, bn=False):
    layers = [nn.Linear(in_dim, 512)]
    if bn:
        layers.append(nn.BatchNorm1d(512))
    layers += [nn.ReLU(), nn.Dropout(0.2), nn.Linear(512, out_dim), final]
    return nn.Sequential(*layers)


_HEAD_SPECS = (("pose_head_1", 4, "softmax"), ("pose_head_2", 4, "softmax"), ("pose_head_3", 4, "softmax"),
               ("intrctn_head_1", 2, "sigmoid"), ("intrctn_head_2", 4, "sigmoid"), ("intrctn_head_3", 7, "sigmoid"),
               ("intrctn_head_4", 5, "sigmoid"))


class Actionhead(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        for name, k, kind in _HEAD_SPECS:
            setattr(self, name, _head(1024, k, nn.Softmax(dim=1) if kind == "softmax" else nn.Sigmoid(), bn=True))

    def forward(self, x):
        return tuple(getattr(self, name)(x) for name, _, _ in _HEAD_SPECS)


# FUSION values whose scenes can be evaluated together on packed rows (forward_packed); the rest goes scene by scene.
# MODALITY 'RGB' / 'LiDAR' (one backbone, no fusion) ignore FUSION when fusing but NOT in the adjacency, which the reference
# keys on FUSION alone: they take the packed route unless FUSION is one of _BILINEAR_ADJACENCY.
_PACKED_FUSIONS = ('Attention_mat', 'sum', 'Attention_normal', 'Attention_max', 'Attention_multi', 'Attention_gaussian',
                   'crossAtt', 'catandAtt')
_BILINEAR_ADJACENCY = ('Attention', 'Attention_sum')     # A_theta = sigmoid(phi sigma^T + sigma phi^T): no packed form
_PRESENT = {'Multi': (True, True), 'RGB': (True, False), 'LiDAR': (False, True)}   # MODALITY -> (RGB rows, LiDAR rows) used

_PAIR_LOCAL_CACHE = {}


def _pair_local(counts, n_max, device):
    """(pairs,) int64: (s * n_max + i) * n_max + j of every packed pair (s, i, j), its place in a (S, n_max, n_max) tensor
    viewed flat.  Built on the host once per count tuple and cached, like scene_layout."""
    key = (tuple(counts), int(n_max), str(device))
    hit = _PAIR_LOCAL_CACHE.get(key)
    if hit is None:
        parts = []
        for s, n in enumerate(counts):
            i = torch.arange(n, dtype=torch.int64)
            parts.append((((s * n_max + i) * n_max)[:, None] + i[None, :]).reshape(-1))
        hit = (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)).to(device)
        if len(_PAIR_LOCAL_CACHE) < 64:
            _PAIR_LOCAL_CACHE[key] = hit
    return hit


class GAR_Fusion_Net3(nn.Module):
    def __init__(self, cfg) -> None:
        super().__init__()
        self.cfg = cfg
        if cfg.EUCLIDEAN:
            self.D_embed = nn.Sequential(nn.Linear(2, 1), nn.Sigmoid())
        else:
            self.D_embed = nn.Sequential(nn.Linear(2, 4), nn.ReLU(), nn.Linear(4, 1), nn.Sigmoid())
        if cfg.get("Social_Layer"):
            self.social_layer = nn.Sequential(nn.Linear(int(cfg.FEATURE_DIM / 2), 256), nn.ReLU(), nn.Linear(256, 128))
        if cfg.get("Social_Encoder"):
            self.social_layer = nn.TransformerEncoderLayer(d_model=512, nhead=8)
        for name, k, kind in _HEAD_SPECS:  # individual actions: Softmax for poses, Sigmoid for interactions
            setattr(self, name, _head(cfg.FEATURE_DIM, k, nn.Softmax(dim=1) if kind == "softmax" else nn.Sigmoid()))
        for name, k, _ in _HEAD_SPECS:     # social-group activity: all Sigmoid (:1166-1173)
            setattr(self, "SG_" + name, _head(cfg.HIDDEN_DIM, k, nn.Sigmoid()))
        fus = cfg.FUSION
        two = {"Attention_mat": FusionAttention_mat, "Attention_normal": FusionAttention, "Attention_pe": FusionAttention_pe,
               "Attention_MMCA_sty": FusionAttention_MMCA_sty}
        if fus in two:
            self.AttFusModule1 = two[fus](sigma=cfg.SIGMA)
            self.AttFusModule2 = two[fus](sigma=cfg.SIGMA)
        elif fus == "Attention_multi":
            self.AttFusModule1 = FusionAttention3(sigma=3.)
            self.AttFusModule2 = FusionAttention2(sigma=1.)
        elif fus == "Attention_multi_cat":
            sig = {2: (1., 0.5), 4: (5., 3., 1., 0.5)}.get(cfg.get("Layer"), ())
            for i, s in enumerate(sig):
                setattr(self, "AttFusModule%d" % (i + 1), FusionAttention3(sigma=s))
        elif fus == "Attention_gaussian":
            for i in range(4):
                setattr(self, "AttFusModule%d" % (i + 1), FusionAttention_gaussian(sigma=3))
        elif fus in ("Attention", "Attention_max", "Attention_sum"):
            self.AttFusModule = (FusionAttention_sum if fus == "Attention_sum" else FusionAttention2)(sigma=cfg.SIGMA)
            self.phi = nn.Sequential(nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 32))
            self.sigma = nn.Sequential(nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 32))
        elif fus == "Attention_concat":
            self.AttFusModule = FusionAttention_cat(sigma=cfg.SIGMA)
        elif fus == 'catandAtt':
            self.Att = nn.MultiheadAttention(512, 8)
            self.FL = nn.Linear(1024, 512); self.LN = nn.LayerNorm([512])
            self.FL2 = _ffn(512); self.LN2 = nn.LayerNorm([512])
        elif fus == "crossAtt":
            self.AttFusModule = cross_attention_fusion()
            self.D_embed = nn.Sequential(nn.Linear(32, 8), nn.ReLU(), nn.Linear(8, 1), nn.Sigmoid())
            self.F_embed = nn.Linear(512, 30)
        self.f_dim = cfg.FEATURE_DIM
        self.card_net = nn.Sequential(nn.Linear(513, 512), nn.ReLU(), nn.Linear(512, 1))
        self.bn_rgb = nn.BatchNorm1d(512)
        self.bn_lidar = nn.BatchNorm1d(512)
        if cfg.sim == "Graph":
            self.phi = nn.Sequential(nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 32))
            self.sigma = nn.Sequential(nn.Linear(512, 32), nn.ReLU(), nn.Linear(32, 32))
        elif cfg.sim == "Graph2":
            self.phi = nn.Sequential(nn.Linear(515, 8)); self.sigma = nn.Sequential(nn.Linear(515, 8))
        elif cfg.sim == "Graph4":
            self.phi = nn.Sequential(nn.Linear(515, 8))

    # ------------------------------------------------------------------ small helpers
    def get_f_dim(self):
        return self.f_dim

    def get_num_person(self, person_id):
        return [len(torch.unique(person_id[i])) - 1 for i in range(person_id.shape[0])]

    def Get_similarity_Mat(self, fusion_feature, bboxe3d=None):
        """D_v: similarity between individual features, (N, N)."""
        sim = self.cfg.sim
        if sim == "Graph":
            phi, sigma = self.phi(fusion_feature), self.sigma(fusion_feature)
            return torch.mm(phi, sigma.T) + torch.mm(sigma, phi.T)
        if sim in ("Graph2", "Graph3", "Graph4"):
            feat = torch.cat((fusion_feature, bboxe3d), dim=-1)
            if sim == "Graph2":
                phi, sigma = self.phi(feat), self.sigma(feat)
                out = torch.sigmoid(torch.mm(phi, sigma.T) + torch.mm(sigma, phi.T))
            elif sim == "Graph3":
                out = torch.sigmoid(torch.mm(feat, feat.T) / feat.shape[1])
            else:
                phi = self.phi(feat)
                out = torch.sigmoid(torch.mm(phi, phi.T))
            return out if self.training else out.fill_diagonal_(1.)
        if self.cfg.get("Social_Layer") or self.cfg.get("Social_Encoder"):
            fusion_feature = self.social_layer(fusion_feature)
        return pairwise_cosine_similarity(fusion_feature, zero_diagonal=False)

    def Get_GIoU_Mat(self, bboxes):
        return TO.generalized_box_iou(bboxes, bboxes)

    # ------------------------------------------------------------------ per-scene pieces
    def _fuse(self, R, L, bboxes_b, bboxes3d_b, b_all3d):
        cfg = self.cfg
        fus = cfg.FUSION
        if cfg.MODALITY == 'RGB':
            return R
        if cfg.MODALITY == 'LiDAR':
            return L
        if fus == 'sum':
            return R + L
        if fus == 'concat':
            return torch.cat((R, L), dim=1)
        if fus == 'crossAtt':
            return self.AttFusModule(R, L)
        if fus == 'catandAtt':
            x = self.FL(torch.concat([R, L], dim=1))
            x = self.LN(x + self.Att(x, x, x)[0])
            return self.LN2(self.FL2(x) + x)
        if fus == 'Attention_normal':
            self.AttFusModule1(R, L, None, None)
            Rp, Lp = self.AttFusModule2(R, L, None, None)   # the reference feeds R, L again (:1435)
            return torch.max(torch.stack((Rp, Lp)), dim=0)[0]
        if fus == 'Attention_pe':
            bb = b_all3d[:, :2]
            Rp, Lp = self.AttFusModule1(R, L, bb)
            Rp, Lp = self.AttFusModule2(Rp, Lp, bb)
            return torch.max(torch.stack((Rp, Lp)), dim=0)[0]
        Dg = TO.generalized_box_iou(bboxes_b, bboxes_b)
        De = pairwise_euclidean_distance(bboxes3d_b, zero_diagonal=True)
        if fus == 'Attention_MMCA_sty':
            dist = self.cfg.get("Gaussian") == True  # noqa: E712
            Rp, Lp = self.AttFusModule1(R, L, Dg, De, dist)
            Rp, Lp = self.AttFusModule2(Rp, Lp, Dg, De, dist)
            return torch.max(torch.stack((Rp, Lp)), dim=0)[0]
        if fus in ('Attention', 'Attention_concat', 'Attention_sum', 'Attention_max'):
            return self.AttFusModule(R, L, Dg, De)
        if fus in ('Attention_mat', 'Attention_gaussian'):
            Rp, Lp = R, L
            for i in range(2 if fus == 'Attention_mat' else 4):
                Rp, Lp = getattr(self, "AttFusModule%d" % (i + 1))(Rp, Lp, Dg, De)
            return torch.max(torch.stack((Rp, Lp)), dim=0)[0]
        if fus == 'Attention_multi':
            Rp, Lp = self.AttFusModule1(R, L, Dg, De)
            return self.AttFusModule2(Rp, Lp, Dg, De)
        raise NotImplementedError("GAR_MODEL.FUSION = %r" % fus)

    def _adjacency(self, fusion_feature_b, Dv, Dg, De, n):
        cfg = self.cfg
        if cfg.FUSION in ('Attention', 'Attention_sum'):
            phi, sigma = self.phi(fusion_feature_b), self.sigma(fusion_feature_b)
            return torch.sigmoid(torch.mm(phi, sigma.T) + torch.mm(sigma, phi.T))
        if cfg.FUSION == "crossAtt":
            a = self.F_embed(fusion_feature_b)
            diff = a.unsqueeze(1).repeat([1, n, 1]) - a.unsqueeze(0).repeat([n, 1, 1])
            feat = torch.cat((diff, Dg.unsqueeze(-1), De.unsqueeze(-1)), dim=-1).reshape(-1, 32)
            return self.D_embed(feat).reshape(n, n)
        if cfg.sim in ("Graph2", "Graph3", "Graph4"):
            return Dv
        # both remaining branches of the reference (:1555-1571) feed [Dv, Dg]; De is computed but
        # not concatenated even when EUCLIDEAN is set
        feat = torch.cat((Dv.unsqueeze(-1), Dg.unsqueeze(-1)), dim=-1).reshape(-1, 2)
        return self.D_embed(feat).reshape(n, n)

    def _predicted_groups(self, A_theta):
        """Group id of each actor = first column of its thresholded adjacency row (:1580-1592);
        evaluated on the device (the reference calls .item() per row)."""
        tmp = A_theta.detach().clone().fill_diagonal_(1.)
        n = tmp.shape[0]
        cols = torch.arange(n, device=tmp.device).expand(n, n)
        return torch.where(tmp >= 0.5, cols, torch.full_like(cols, n)).min(dim=1).values

    @staticmethod
    def _group_max_pool(feats, group_id):
        """Max over the members of each actor's group, broadcast back to the actors."""
        n, d = feats.shape
        pooled = torch.full((n, d), float("-inf"), device=feats.device, dtype=feats.dtype)
        pooled = pooled.scatter_reduce(0, group_id.view(-1, 1).expand(-1, d), feats, reduce="amax", include_self=True)
        return pooled[group_id]

    _OUT_DIMS = (4, 4, 4, 2, 4, 7, 5)

    def forward(self, RGB_feature, LiDAR_feature, bboxes, bboxes3d, social_group_id, person_id):
        """RGB_feature / LiDAR_feature (B, MAX_NUM_PROPOSAL, 512), bboxes (B, MNP, 4) xyxy,
        bboxes3d (B, MNP, 7) -> 16 zero-padded tensors in the order of reference :1696."""
        counts = self._scene_counts(RGB_feature, LiDAR_feature, person_id)
        if counts is None:
            return self.forward_per_scene(RGB_feature, LiDAR_feature, bboxes, bboxes3d, social_group_id, person_id)
        if self.cfg.MODALITY == 'Multi' and self.cfg.FUSION == 'Attention_mat' and all(c == counts[0] for c in counts):
            return self._forward_batched(RGB_feature, LiDAR_feature, bboxes, bboxes3d, person_id, counts[0])
        return self._forward_ragged(RGB_feature, LiDAR_feature, bboxes, bboxes3d, counts)

    def forward_per_scene(self, RGB_feature, LiDAR_feature, bboxes, bboxes3d, social_group_id, person_id):
        cfg = self.cfg
        person_num = self.get_num_person(person_id)
        _B, MNP = person_id.shape
        device = RGB_feature.device if cfg.MODALITY == 'RGB' else LiDAR_feature.device
        A_list = torch.zeros([_B, MNP, MNP], device=device)
        ind_lists = [torch.zeros([_B, MNP, k], device=device) for k in self._OUT_DIMS]
        sg_lists = [torch.zeros([_B, MNP, k], device=device) for k in self._OUT_DIMS]
        card_list = torch.zeros([_B, 1], device=device)
        for b in range(_B):
            n = person_num[b]
            R = RGB_feature[b, :n, :] if cfg.MODALITY in ('RGB', 'Multi') else None
            L = LiDAR_feature[b, :n, :] if cfg.MODALITY in ('LiDAR', 'Multi') else None
            if cfg.FEAT_NORM:
                R = self.bn_rgb(R) if R is not None else None
                L = self.bn_lidar(L) if L is not None else None
            bboxes_b = bboxes[b, :n, :]
            bboxes3d_b = bboxes3d[b, :n, :3]
            fused = self._fuse(R, L, bboxes_b, bboxes3d_b, bboxes3d[b, :n])
            Dv = self.Get_similarity_Mat(fused, bboxes3d_b)
            Dg = TO.generalized_box_iou(bboxes_b, bboxes_b)
            De = pairwise_euclidean_distance(bboxes3d_b, zero_diagonal=True)
            A_theta = self._adjacency(fused, Dv, Dg, De, n)
            if not self.training:
                A_theta = A_theta.fill_diagonal_(1.)
            group_id = self._predicted_groups(A_theta)
            if cfg.get("Action_concat"):
                fused = torch.cat((R, L), dim=1)
            pooled = self._group_max_pool(fused, group_id)
            res_feature = torch.cat([fused, pooled], dim=-1)
            sg_features = fused if cfg.get("sg_feat_org") else pooled
            if cfg.get("Non_concat"):
                res_feature = fused
            if cfg.get("ind_action_concat"):
                res_feature = {'LiDAR': L, 'RGB': R}.get(cfg.MODALITY, None)
                if res_feature is None:
                    res_feature = torch.cat([R, L], dim=-1)
            for (name, _, _), dst in zip(_HEAD_SPECS, ind_lists):
                dst[b, :n] = getattr(self, name)(res_feature)
            for (name, _, _), dst in zip(_HEAD_SPECS, sg_lists):
                dst[b, :n] = getattr(self, "SG_" + name)(sg_features)
            card_feature = torch.cat((fused.max(dim=0, keepdim=True)[0], A_theta.sum().reshape([1, 1])), dim=1)
            card_list[b] = self.card_net(card_feature)
            A_list[b, :n, :n] = A_theta
        return (A_list, *ind_lists, *sg_lists, card_list)

    # ------------------------------------------------------------------ batched route
    def _scene_counts(self, RGB_feature, LiDAR_feature, person_id):
        """Actors per scene (host ints) when the batch can take a batched route -- _forward_batched for equal counts under
        Attention_mat, _forward_ragged otherwise -- and None when it goes scene by scene: a configuration outside
        _scene_counts_ok (the shipped one and the other FUSION values of _PACKED_FUSIONS pass), valid
        slots that are not the leading columns, a scene of fewer than 2 (BatchNorm1d raises there, and so does the per-scene
        route) or more than MGAR_DAFM_MAX_N actors, or an empty batch.  The caller can promise the counts and spare the host
        read: `uniform_actor_count` (one int for every scene) or `actor_counts` (a sequence of host ints, one per scene); where
        both are set, `uniform_actor_count` is the one that holds.  A promised count is taken as given: a caller that promises
        as many actors as there are slots gets them all, where the derived count of such a scene is one short (below)."""
        use_r, use_l = _PRESENT.get(self.cfg.MODALITY, (True, True))
        present = [t for t, used in ((RGB_feature, use_r), (LiDAR_feature, use_l)) if used]    # a single modality: the other
        if any(t is None for t in present) or not self._scene_counts_ok([2]):                  # tensor may be None
            return None
        S, MNP = person_id.shape
        if S == 0:
            return None
        n = getattr(self, "uniform_actor_count", None)
        if n:                                           # caller's promise: skips the host read below
            return [int(n)] * S
        counts = getattr(self, "actor_counts", None)
        if counts is not None:                          # the same promise, one count per scene
            counts = [int(c) for c in counts]
            if len(counts) != S:
                raise ValueError("actor_counts promises %d scenes, the batch has %d" % (len(counts), S))
        else:
            # the valid slots are person_id >= 0 and must be the leading columns; one host read for counts and flag together
            valid = person_id >= 0
            cnt = valid.sum(dim=1)
            leading = (valid == (torch.arange(MNP, device=person_id.device)[None, :] < cnt[:, None])).all()
            # a scene without a single -1 slot: the reference counts len(unique(person_id)) - 1 (get_num_person), one actor
            # short, and so does the per-scene route; the last slot is dropped here too
            cnt = cnt - (cnt == MNP).to(cnt.dtype)
            host = torch.cat((cnt, leading.view(1).to(cnt.dtype))).tolist()
            if not host[-1]:
                return None
            counts = host[:-1]
        if not self._scene_counts_ok(counts) or min(t.shape[1] for t in present) < max(counts):
            return None
        return counts

    def _scene_counts_ok(self, counts):
        """Whether scenes of these actor counts can take a batched route under this configuration."""
        cfg = self.cfg
        # Multi: the fusions with a packed form, under FEAT_NORM; one modality: with FEAT_NORM or without it, under every
        # FUSION whose adjacency _adjacency_packed mirrors
        ok = (((cfg.MODALITY == 'Multi' and cfg.FUSION in _PACKED_FUSIONS and cfg.FEAT_NORM)
               or (cfg.MODALITY in ('RGB', 'LiDAR') and cfg.FUSION not in _BILINEAR_ADJACENCY))
              and cfg.sim == 'cosine' and cfg.get("ind_action_concat") and not cfg.get("sg_feat_org") and not cfg.get("Social_Layer")
              and not cfg.get("Social_Encoder") and not cfg.get("Action_concat") and not cfg.get("DISABLE_BATCHED"))
        return bool(ok) and len(counts) > 0 and min(counts) >= 2 and max(counts) <= 128

    def _scene_bn(self, bn, x):
        """BatchNorm1d applied to every scene separately (per-scene statistics, like the reference's
        loop), for x (S, N, C).  Running statistics receive the same sequence of EMA updates."""
        if not self.training:
            return _eval_bn(bn, x)
        mean = x.mean(dim=1, keepdim=True)
        var = x.var(dim=1, unbiased=False, keepdim=True)
        y = (x - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
        with torch.no_grad():
            s, n = x.shape[0], x.shape[1]
            m = bn.momentum
            w = m * (1 - m) ** torch.arange(s - 1, -1, -1, device=x.device, dtype=x.dtype)   # scene 0 decays most
            keep = (1 - m) ** s
            bn.running_mean.mul_(keep).add_((w[:, None] * mean[:, 0]).sum(0))
            bn.running_var.mul_(keep).add_((w[:, None] * var[:, 0] * (n / (n - 1))).sum(0))
            bn.num_batches_tracked += s
        return y

    def _forward_batched(self, RGB_feature, LiDAR_feature, bboxes, bboxes3d, person_id, n=None):
        S, MNP = person_id.shape
        n = n or getattr(self, "uniform_actor_count", None) or int((person_id[0] >= 0).sum().item())
        device = RGB_feature.device
        R = self._scene_bn(self.bn_rgb, RGB_feature[:, :n, :])
        L = self._scene_bn(self.bn_lidar, LiDAR_feature[:, :n, :])
        bb = bboxes[:, :n, :]
        ctr = bboxes3d[:, :n, :3]
        # distance matrices for all scenes
        cd = ctr.double()
        sq = (cd * cd).sum(-1)
        De = (sq[:, :, None] + sq[:, None, :] - 2 * cd @ cd.transpose(1, 2)).clamp(min=0).sqrt().to(R.dtype)
        De = De * (1 - torch.eye(n, device=device, dtype=R.dtype))
        so, do = scene_offsets([n] * S, device)
        Rf, Lf = R.reshape(S * n, -1), L.reshape(S * n, -1)
        de_flat = De.reshape(-1)
        Rp, Lp = self.AttFusModule1.forward_stacked(Rf, Lf, de_flat, so, do)
        Rp, Lp = self.AttFusModule2.forward_stacked(Rp, Lp, de_flat, so, do)
        fused = torch.max(Rp, Lp).view(S, n, -1)
        Dg = torch.stack([TO.generalized_box_iou(bb[s], bb[s]) for s in range(S)]) if S <= 4 else _giou_batched(bb)
        self._tail_group_id = None
        if scene_tail_ops.scene_tail_plan(self, fused.view(S * n, -1), [n] * S) is not None:
            # eval mode: the whole tail behind the fused rows in one launch (scene_tail_ops); Dg stays the tensor above
            lay = scene_layout([n] * S, MNP, device)
            A_list, self._tail_group_id, sg_features, card_feature = scene_tail_ops.scene_tail_eval(
                fused.view(S * n, -1), Dg.reshape(-1), lay, self.D_embed)
            res_feature = torch.cat([Rf, Lf], dim=-1)
            outs = []
            for prefix, feat in (("", res_feature), ("SG_", sg_features)):
                outs += self._heads_stacked(prefix, feat, S, n, MNP)
            return (A_list, *outs, self.card_net(card_feature))
        fn = fused / fused.norm(dim=2, keepdim=True)
        Dv = fn @ fn.transpose(1, 2)
        A_theta = self.D_embed(torch.stack((Dv, Dg), dim=-1).reshape(-1, 2)).reshape(S, n, n)
        eye = torch.eye(n, device=device, dtype=torch.bool)
        if not self.training:
            A_theta = A_theta.masked_fill(eye, 1.)
        tmp = A_theta.detach().masked_fill(eye, 1.)
        cols = torch.arange(n, device=device).expand(S, n, n)
        group_id = torch.where(tmp >= 0.5, cols, torch.full_like(cols, n)).min(dim=2).values      # (S, n)
        gflat = (group_id + torch.arange(S, device=device)[:, None] * n).reshape(-1)
        sg_features = self._group_max_pool(fused.reshape(S * n, -1), gflat)
        res_feature = torch.cat([Rf, Lf], dim=-1)
        outs = []
        for prefix, feat in (("", res_feature), ("SG_", sg_features)):
            outs += self._heads_stacked(prefix, feat, S, n, MNP)
        card_feature = torch.cat((fused.max(dim=1)[0], A_theta.sum(dim=(1, 2)).view(S, 1)), dim=1)
        card_list = self.card_net(card_feature)
        A_list = torch.zeros([S, MNP, MNP], device=device, dtype=A_theta.dtype)
        A_list[:, :n, :n] = A_theta
        return (A_list, *outs, card_list)

    def _forward_ragged(self, RGB_feature, LiDAR_feature, bboxes, bboxes3d, counts):
        """The batched route for scenes of unequal actor counts: the valid rows of the padded inputs, packed."""
        S, MNP = bboxes.shape[0], bboxes.shape[1]
        device = bboxes.device
        use_r, use_l = _PRESENT.get(self.cfg.MODALITY, (True, True))

        def rows_of(t):                                 # the padded width is each tensor's own
            return t.reshape(S * t.shape[1], t.shape[2])[scene_layout(counts, t.shape[1], device).row_slot]
        return self.forward_packed(rows_of(RGB_feature) if use_r else None, rows_of(LiDAR_feature) if use_l else None,
                                   rows_of(bboxes), rows_of(bboxes3d)[:, :3], counts, MNP)

    def _packed_bn(self, bn, x, scene_off):
        if not self.training:
            return _eval_bn(bn, x)
        return scene_batch_norm(x, bn.weight, bn.bias, scene_off, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                bn.eps, bn.momentum)

    def _fuse_packed(self, R, L, de, dg, so, do, pairs=None):
        """`_fuse` for the packed rows of all scenes (the configurations of _PACKED_FUSIONS): de, dg are the scenes' flat
        (n_s, n_s) matrices, so / do their offsets, pairs = sum n_s^2 (host int; None: read back from the device).  Under
        MODALITY 'RGB' / 'LiDAR' the absent side is None and the present rows are the result."""
        fus = self.cfg.FUSION
        if self.cfg.MODALITY == 'RGB':
            return R
        if self.cfg.MODALITY == 'LiDAR':
            return L
        if fus == 'crossAtt':
            return self.AttFusModule.forward_stacked(R, L, so, do, packed_pairs(so) if pairs is None else pairs)
        if fus == 'catandAtt':
            x = self.FL(torch.cat([R, L], dim=1))
            x = self.LN(x + scene_multihead_attention(self.Att, x, x, x, so, do, packed_pairs(so) if pairs is None else pairs))
            return self.LN2(self.FL2(x) + x)
        if fus == 'Attention_mat':
            Rp, Lp = self.AttFusModule1.forward_stacked(R, L, de, so, do)
            Rp, Lp = self.AttFusModule2.forward_stacked(Rp, Lp, de, so, do)
            return torch.max(Rp, Lp)
        if fus == 'sum':
            return R + L
        if fus == 'Attention_normal':
            # module 2 on the ORIGINAL R, L (reference :1453); module 1's result is discarded there, so it is not
            # evaluated here and its parameters stay without a gradient, as on the per-scene route
            return torch.max(*self.AttFusModule2.forward_stacked(R, L, None, None, so, do, pairs))
        if fus == 'Attention_max':
            return self.AttFusModule.forward_stacked(R, L, de, dg, so, do, pairs)
        if fus == 'Attention_multi':
            Rp, Lp = self.AttFusModule1.forward_stacked(R, L, de, dg, so, do, pairs)
            return self.AttFusModule2.forward_stacked(Rp, Lp, de, dg, so, do, pairs)
        if fus == 'Attention_gaussian':
            Rp, Lp = R, L
            for i in range(4):
                Rp, Lp = getattr(self, "AttFusModule%d" % (i + 1)).forward_stacked(Rp, Lp, de, dg, so, do, pairs)
            return torch.max(Rp, Lp)
        raise NotImplementedError("GAR_MODEL.FUSION = %r has no packed route" % fus)

    def _adjacency_packed(self, fused, de, dg, lay):
        """`_adjacency` for the packed pairs of all scenes -> (sum n_s^2,).  Like `_adjacency` it is keyed on FUSION alone,
        whatever MODALITY is; the bilinear form of _BILINEAR_ADJACENCY has no packed mirror and raises."""
        if self.cfg.FUSION in _BILINEAR_ADJACENCY:
            raise NotImplementedError("GAR_MODEL.FUSION = %r: its adjacency has no packed route" % self.cfg.FUSION)
        if self.cfg.FUSION == 'crossAtt':
            # reference :1532-1544: [a_i - a_j, Dg_ij, De_ij] through the 32 -> 8 -> 1 D_embed; Dv is not read, so no Gram
            # matrix.  The differences are formed on a (S, n_max, n_max) grid and the packed pairs gathered from it: every
            # index below hits each of its targets once, so the backward sums in a fixed order (plain torch: n^2 * 32 work).
            # Gathering a[i] - a[j] straight from the rows would scatter-add n gradients into every row in the backward, in
            # no fixed order.  The price is the grid: S * n_max^2 * 30 floats, in the forward and again in the backward --
            # 15 MB at 120 scenes of 32 actors, 236 MB if ONE of 120 scenes holds 128.
            S, n_max = len(lay.counts), lay.n_max
            a = self.F_embed(fused)
            a = a.new_zeros(S * n_max, a.shape[1]).index_copy(0, lay.row_local, a).view(S, n_max, -1)
            diff = (a[:, :, None, :] - a[:, None, :, :]).reshape(S * n_max * n_max, -1)
            diff = diff.index_select(0, _pair_local(lay.counts, n_max, fused.device))
            return self.D_embed(torch.cat((diff, dg[:, None], de[:, None]), dim=1)).reshape(-1)
        fn = fused / fused.norm(dim=1, keepdim=True)
        Dv = scene_gram(fn, lay.scene_off, lay.de_off, lay.pairs)
        return self.D_embed(torch.stack((Dv, dg), dim=-1)).reshape(-1)

    def forward_packed(self, R, L, bb, ctr, counts, MNP):
        """R, L (rows, 512), bb (rows, 4) xyxy, ctr (rows, 3): the rows of all scenes stacked, scene s holding counts[s] of
        them (host ints, each 2..MGAR_DAFM_MAX_N) -> the 16 zero-padded (S, MNP, .) tensors of forward().  Every step is one
        launch sequence for all scenes; with a count tuple seen before, nothing reads from or writes to the host.  Under
        MODALITY 'RGB' / 'LiDAR' the absent one of R, L is None (and ignored if given)."""
        cfg = self.cfg
        use_r, use_l = _PRESENT.get(cfg.MODALITY, (True, True))
        R, L = (R if use_r else None), (L if use_l else None)
        S, device = len(counts), bb.device
        lay = scene_layout(counts, MNP, device)
        so, do = lay.scene_off, lay.de_off
        if cfg.FEAT_NORM:                               # BatchNorm on what is present, as forward_per_scene
            R = None if R is None else self._packed_bn(self.bn_rgb, R, so)
            L = None if L is None else self._packed_bn(self.bn_lidar, L, so)
        de, dg = scene_pair_geometry(ctr, bb, so, do, lay.pairs)
        fused = self._fuse_packed(R, L, de, dg, so, do, lay.pairs)
        res_feature = torch.cat([R, L], dim=-1) if use_r and use_l else (R if use_r else L)
        self._tail_group_id = None
        if scene_tail_ops.scene_tail_plan(self, fused, counts) is not None:
            # eval mode: the whole tail behind the fused rows in one launch (scene_tail_ops)
            A_list, self._tail_group_id, sg_features, card_feature = scene_tail_ops.scene_tail_eval(fused, dg, lay, self.D_embed)
            outs = []
            for prefix, feat in (("", res_feature), ("SG_", sg_features)):
                outs += self._heads_stacked(prefix, feat, S, None, MNP, lay.row_slot)
            return (A_list, *outs, self.card_net(card_feature))
        A_theta = self._adjacency_packed(fused, de, dg, lay)                                     # (sum n_s^2,)
        if not self.training:
            A_theta = A_theta.index_fill(0, lay.diag_index, 1.)
        A_list = torch.zeros(S * MNP * MNP, device=device, dtype=A_theta.dtype).index_put((lay.pair_index,), A_theta)
        A_list = A_list.view(S, MNP, MNP)
        # group ids on the padded tensor: padding entries are 0 < 0.5 and can never be picked; diagonal 1 for valid rows only
        tmp = A_list.detach().reshape(-1).index_fill(0, lay.pair_index[lay.diag_index], 1.).view(S, MNP, MNP)
        cols = torch.arange(MNP, device=device).expand(S, MNP, MNP)
        group_id = torch.where(tmp >= 0.5, cols, torch.full_like(cols, MNP)).min(dim=2).values  # (S, MNP)
        gflat = group_id.reshape(-1)[lay.row_slot] + so.long()[lay.row_scene]
        sg_features = self._group_max_pool(fused, gflat)
        outs = []
        for prefix, feat in (("", res_feature), ("SG_", sg_features)):
            outs += self._heads_stacked(prefix, feat, S, None, MNP, lay.row_slot)
        col_max = fused.new_full((S * lay.n_max, fused.shape[1]), float("-inf")).index_copy(0, lay.row_local, fused)
        col_max = col_max.view(S, lay.n_max, -1).max(dim=1)[0]
        card_feature = torch.cat((col_max, A_list.sum(dim=(1, 2)).view(S, 1)), dim=1)            # padding adds exact zeros
        card_list = self.card_net(card_feature)
        return (A_list, *outs, card_list)

    def _heads_stacked(self, prefix, feat, S, n, MNP, slot=None):
        """The seven heads that share `feat` (Linear -> ReLU -> Dropout -> Linear -> softmax | sigmoid each,
        reference :1160-1173) evaluated together: one GEMM over the stacked first layers, one dropout mask, one
        block-diagonal GEMM for the second layers, one softmax over the three pose heads and one sigmoid over the
        rest -- ~20 launches instead of ~110 (and as many again in the backward), which is what a rank that holds
        a single clip is made of.  Returns the reference's per-head (S, MNP, k) tensors (views of one buffer).
        feat holds n rows per scene, or, with `slot`, packed rows whose places in (S * MNP) `slot` gives."""
        heads = [getattr(self, prefix + name) for name, _, _ in _HEAD_SPECS]
        if any(len(h) != 5 for h in heads):      # a head with BatchNorm: not stackable
            outs = []
            for h, (_, k, _) in zip(heads, _HEAD_SPECS):
                o = torch.zeros([S, MNP, k], device=feat.device, dtype=feat.dtype)
                if slot is None:
                    o[:, :n] = h(feat).view(S, n, k)
                else:
                    o = o.view(S * MNP, k).index_copy(0, slot, h(feat)).view(S, MNP, k)
                outs.append(o)
            return outs
        ks = [k for _, k, _ in _HEAD_SPECS]
        hid_dim = heads[0][0].out_features
        if not self.training and not torch.is_grad_enabled():
            # a frozen model: the stacked parameters are built once (the same ops, the same bits) and reused
            w1, b1, w2, b2 = scene_tail_ops.stacked_head_params(self, prefix, heads, ks)
            logits = F.linear(F.relu(F.linear(feat, w1, b1)), w2, b2)
        else:
            w1 = torch.cat([h[0].weight for h in heads], 0)
            b1 = torch.cat([h[0].bias for h in heads], 0)
            hid = F.dropout(F.relu(F.linear(feat, w1, b1)), heads[0][2].p, self.training)        # (S*n, 7*hid)
            w2 = feat.new_zeros(sum(ks), len(heads) * hid_dim)                                    # block diagonal
            row = 0
            for i, (h, k) in enumerate(zip(heads, ks)):
                w2[row:row + k, i * hid_dim:(i + 1) * hid_dim] = h[3].weight
                row += k
            logits = F.linear(hid, w2, torch.cat([h[3].bias for h in heads], 0))                  # (S*n, sum k)
        n_soft = sum(1 for _, _, kind in _HEAD_SPECS if kind == "softmax" and prefix == "")       # SG_ heads: all sigmoid
        k_soft = sum(ks[:n_soft])
        assert all(k == ks[0] for k in ks[:n_soft])
        parts = []
        if n_soft:
            parts.append(torch.softmax(logits[:, :k_soft].reshape(-1, n_soft, ks[0]), dim=2).reshape(-1, k_soft))
        parts.append(torch.sigmoid(logits[:, k_soft:]))
        full = torch.zeros([S, MNP, sum(ks)], device=feat.device, dtype=feat.dtype)
        if slot is None:
            full[:, :n] = torch.cat(parts, 1).view(S, n, sum(ks))
        else:
            full = full.view(S * MNP, sum(ks)).index_copy(0, slot, torch.cat(parts, 1)).view(S, MNP, sum(ks))
        outs, col = [], 0
        for k in ks:
            outs.append(full[:, :, col:col + k])
            col += k
        return outs

    def getloss(self, ):
        return


def _eval_bn(bn, x):
    """Eval-mode BatchNorm1d of the batched routes, (x - mean) / sqrt(var + eps) * weight + bias as ever, with the square
    root cached on the module (eval_route.cached under running_var, with eps in the key): the same bits, two launches fewer
    per call on a frozen model."""
    rv = bn.running_var
    std = cached(bn, "_mgar_eval_std", (rv,), lambda: torch.sqrt(rv + bn.eps), extra=(float(bn.eps),))
    return (x - bn.running_mean) / std * bn.weight + bn.bias


def _giou_batched(bb):
    """generalized_box_iou of every scene with itself: bb (S, n, 4) -> (S, n, n)."""
    area = (bb[..., 2] - bb[..., 0]) * (bb[..., 3] - bb[..., 1])
    lt = torch.max(bb[:, :, None, :2], bb[:, None, :, :2]); rb = torch.min(bb[:, :, None, 2:], bb[:, None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area[:, :, None] + area[:, None, :] - inter
    lti = torch.min(bb[:, :, None, :2], bb[:, None, :, :2]); rbi = torch.max(bb[:, :, None, 2:], bb[:, None, :, 2:])
    whi = (rbi - lti).clamp(min=0)
    areai = whi[..., 0] * whi[..., 1]
    return inter / union - (areai - union) / areai


class GAR_Fusion_ALL(nn.Module):
    def __init__(self, cfg, dataset):
        super().__init__()
        self.cfg = cfg
        self.num_boxes = cfg.DATALOADER.train.augmentation.num_boxes
        self.modality = cfg.GAR_MODEL.MODALITY
        if self.modality in ("RGB", "Multi"):
            self.RGB_backbone = RGB_Backbone(cfg=cfg.RGB_BACKBONE)
        if self.modality in ("LiDAR", "Multi"):
            self.LiDAR_backbone = LiDAR_Backbone(cfg=cfg, dataset=dataset)
        self.GAR_model = GAR_Fusion_Net3(cfg=cfg.GAR_MODEL)

    def check(self):
        for name, param in self.GAR_model.named_parameters():
            print(name, param.requires_grad)

    def forward(self, batch):
        (images, bboxes, pcs, bboxes3d, bboxes_num, person_id, social_group_id, seq_id, frame_id, action,
         social_group_activity, data_dict) = batch
        rgb_feature = lidar_feature = None
        if self.modality in ("RGB", "Multi"):
            _B, _T, _C, _H, _W = images.shape
            images = images.view(_B, _C, _T, _H, _W)  # a VIEW, not a permute -- as the reference (:1836)
            rgb_feature = self.RGB_backbone(images, [bboxes[i, :, :] for i in range(bboxes.shape[0])], person_id)
            rgb_feature = rgb_feature.reshape(_B, rgb_feature.shape[0], -1)
        if self.modality in ("LiDAR", "Multi"):
            load_data_to_gpu(data_dict)
            lidar_feature = self.LiDAR_backbone(data_dict)
        return self.GAR_model(rgb_feature, lidar_feature, bboxes, bboxes3d, social_group_id, person_id)


def _legacy(name, why):
    class _Legacy(nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            raise NotImplementedError("%s: %s" % (name, why))
    _Legacy.__name__ = name
    return _Legacy


GARNet = _legacy("GARNet", "legacy experiment built on model.jrdb_act_rep and a `config` module that the reference "
                           "repo does not contain (gat_model.py:1701-1803); not on the MGAR-net hot path")
GARNet_All = _legacy("GARNet_All", "legacy experiment (gat_model.py:1856-1949); not on the MGAR-net hot path")
