"""The benchmark / smoke workload: one MGAR-net training step over a batch of synthetic clips.

The reference has no benchmark; BASELINE.json defines the shape (config c3: 8 clips x 15 frames x
32 actors x 16 384 points, fp32, forward + backward).  What one "clip" is here (frozen builder's
choice, DESIGN.md section "workload"):

  RGB   : the clip's T frames (B, T, 3, H, W) go through I3D once per clip, batch 1, exactly as the
          reference runs it (BATCH_SIZE 1, mil3.yaml:161); centre temporal slice -> RoIAlign of the
          clip's A actor boxes -> non-local block -> Linear -> GATv2 over the actor graph:
          R tokens (A, 512) per clip.
  LiDAR : every one of the clip's T frames is an independent scene of P points with its own A
          actor boxes; all B*T frames form the batch of the PointNet++ stack (SA x 4 + FP x 4:
          FPS, ball query, grouping, three-NN interpolation) and of the per-actor RoI-grid lift
          (6^3 grid points per actor, 3 radii) -> (B*T*A, 216, 96) -> non-local block 3D ->
          Linear(20736, 512): L tokens (A, 512) per frame.
  fuse  : each frame is one scene for GAR_Fusion_Net3 (DAFM x 2, similarity, adjacency, group
          pooling, 14 heads + cardinality) with R of its clip and L of the frame: B*T scenes.
  loss  : a synthetic scalar over all 16 outputs (the reference's JRDB losses need labels and are
          out of scope); backward through everything trainable (I3D is frozen,
          as in the reference) and one Adam step.

Data parallelism: the clip batch is sharded across ranks (one process per GPU); gradients are
all-reduced by DistributedDataParallel over RCCL.
"""
import math
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import synthetic as S
from .pcdet.config import EasyDict

PC_RANGE = [-20.0, -20.0, -2.0, 20.0, 20.0, 2.0]


def lidar_model_cfg(n_points, route="pointnet2"):
    if route == "pointnet2":
        p = n_points
        return EasyDict(
            NAME="PointNet2RoI",
            BACKBONE_3D=dict(
                NAME="PointNet2MSG",
                # OpenPCDet's stock PointNet2MSG plan, with the level sizes tied to the cloud size
                SA_CONFIG=dict(NPOINTS=[p // 4, p // 16, p // 64, p // 256],
                               RADIUS=[[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]],
                               NSAMPLE=[[16, 32], [16, 32], [16, 32], [16, 32]],
                               MLPS=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]],
                                     [[128, 196, 256], [128, 196, 256]], [[256, 256, 512], [256, 384, 512]]]),
                FP_MLPS=[[128, 128], [256, 256], [512, 512], [512, 512]],
                # nothing downstream of the trunk reads the stacked (P, C) copy on the device: the RoI head takes the
                # channel-major tensor (point_features_cm), so the ~1 GB transposed copy is skipped
                STACKED_POINT_FEATURES=False),
            ROI_HEAD=dict(NAME="PointGridRoIHead",
                          # pooling geometry of mil3.yaml:105-134
                          ROI_GRID_POOL=dict(GRID_SIZE=6, MLPS=[[32, 32], [32, 32], [32, 32]],
                                             POOL_RADIUS=[0.4, 0.8, 1.6], NSAMPLE=[16, 16, 16], POOL_METHOD="max_pool")))
    if route == "voxel":
        layer = lambda r: dict(MLPS=[[32, 32]], QUERY_RANGES=[[4, 4, 4]], POOL_RADIUS=[r], NSAMPLE=[16],  # noqa: E731
                               POOL_METHOD="max_pool")
        return EasyDict(
            NAME="VoxelRCNN", VFE=dict(NAME="MeanVFE"), BACKBONE_3D=dict(NAME="VoxelBackBone8x"),
            ROI_HEAD=dict(NAME="VoxelRCNNHead", CLASS_AGNOSTIC=True, SHARED_FC=[512, 512], DP_RATIO=0.3,
                          ROI_GRID_POOL=dict(FEATURES_SOURCE=["x_conv2", "x_conv3", "x_conv4"], PRE_MLP=True, GRID_SIZE=6,
                                             POOL_LAYERS=dict(x_conv2=layer(0.4), x_conv3=layer(0.8), x_conv4=layer(1.6)))))
    raise ValueError(route)


def model_cfg(n_actors, n_points, gat=True, route="pointnet2", fusion="Attention_mat", modality="Multi"):
    """The shipped configuration (Multimodal_cfg/mil3.yaml) with the synthetic sizes plugged in.  fusion: GAR_MODEL.FUSION, the
    shipped DAFM by default; the ablation variants with fixed sigmas (Attention_multi, Attention_gaussian) take them from
    their classes, SIGMA is for the others.  modality: "Multi", or "RGB" / "LiDAR" for the single-modality baselines, which
    run without feature normalisation (the reference raises on them with FEAT_NORM) and with 512-wide individual heads.
    GAT_module is False in the shipped YAML (:86); the north-star includes the GAT path, so the
    benchmark flips it on (SURVEY.md "facts")."""
    if modality not in ("Multi", "RGB", "LiDAR"):
        raise ValueError("modality: 'Multi', 'RGB' or 'LiDAR', got %r" % (modality,))
    cfg = _model_cfg(n_actors, n_points, gat, route, fusion)
    if modality != "Multi":
        cfg.GAR_MODEL.update(MODALITY=modality, FEAT_NORM=False, FEATURE_DIM=512)
    return cfg


def _model_cfg(n_actors, n_points, gat, route, fusion):
    return EasyDict(
        DATALOADER=dict(train=dict(augmentation=dict(num_boxes=n_actors + 1, image_size=[720, 1280], crop_size=5))),
        RGB_BACKBONE=dict(I3D_FREEZE=True, EMBEDDING_DIM=512, INTER_PERSON=False, GAT_module=bool(gat), two_stage_att=False),
        LiDAR_BACKBONE=dict(CLASS_NAMES=["Pedestrian"], MODEL=lidar_model_cfg(n_points, route),
                            SELF_ATT1=dict(USE=True, DIM=3, INTER_PERSON=False), two_stage_att=False),
        GAR_MODEL=dict(MODALITY="Multi", FUSION=fusion, SIGMA=10, FEAT_NORM=True, EUCLIDEAN=True,
                       ind_action_concat=True, sg_feat_org=False, FEATURE_DIM=1024, HIDDEN_DIM=512, sim="cosine"))


class SyntheticDataset:
    """The attributes pcdet's detector template reads from a dataset (detector3d_template.py:36-44)."""

    def __init__(self, voxel_size=(0.25, 0.25, 0.1)):
        # 160 x 160 x 40 cells over the 40 m x 40 m x 4 m range: 40 cells in z like the shipped grid (mil3.yaml:40,56), which is
        # what VoxelBackBone8x's four z-halvings assume (41 -> 21 -> 11 -> 5 -> 2, spconv_backbone.py:85-117)
        self.class_names = ["Pedestrian"]
        self.point_feature_encoder = EasyDict(num_point_features=4)
        self.point_cloud_range = np.array(PC_RANGE, np.float32)
        self.voxel_size = list(voxel_size)
        self.grid_size = np.round((self.point_cloud_range[3:] - self.point_cloud_range[:3]) / np.array(voxel_size)).astype(np.int64)
        self.depth_downsample_factor = None


def make_batch(seed, n_clips, n_frames, n_actors, n_points, height, width, device, actor_counts=None):
    """Synthetic batch on `device`: dict of tensors (see module docstring for the meaning).  actor_counts: one count per
    clip (every frame of a clip has its clip's count), each at most n_actors: the batch is masked beyond the count as a
    loader pads it -- ids -1, boxes and labels 0 -- and carries the list; None gives the batch as it always was."""
    sc = S.scene_batch(seed, n_clips * n_frames, n_actors, n_points, num_boxes=n_actors + 1, height=height, width=width)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    lab = S.scene_labels(seed + 3, n_clips * n_frames, n_actors, num_boxes=n_actors + 1)
    rng = np.random.default_rng(seed + 1)
    boxes2d = np.zeros((n_clips, n_actors + 1, 4), np.float32)
    for b in range(n_clips):
        boxes2d[b, :n_actors] = S.actor_boxes2d(rng, n_actors, height, width)
    person_id, group_id, action, activity, boxes3d = (sc["person_id"], lab["social_group_id"], lab["action"],
                                                      lab["social_group_activity"], sc["bboxes3d"])
    extra = {}
    if actor_counts is not None:
        actor_counts = [int(c) for c in actor_counts]
        if len(actor_counts) != n_clips or not all(0 <= c <= n_actors for c in actor_counts):
            raise ValueError("actor_counts: one count in 0..%d per clip, got %s" % (n_actors, actor_counts))
        person_id, group_id, action, activity, boxes3d = (np.array(x) for x in (person_id, group_id, action, activity, boxes3d))
        for b, c in enumerate(actor_counts):
            frames = slice(b * n_frames, (b + 1) * n_frames)
            person_id[frames, c:] = -1; group_id[frames, c:] = -1
            action[frames, c:] = 0; activity[frames, c:] = 0; boxes3d[frames, c:] = 0
            boxes2d[b, c:] = 0
        extra["actor_counts"] = actor_counts
    return {
        **extra,
        "images": t(S.images(seed + 2, n_clips, n_frames, height, width)),      # (B, T, 3, H, W)
        "bboxes": t(boxes2d),                                                     # (B, A+1, 4) key-frame boxes
        "points": t(sc["points"]),                                                # (B*T, P, 4)
        "bboxes3d": t(boxes3d),                                                   # (B*T, A+1, 7)
        "person_id": t(person_id),                                                # (B*T, A+1)
        "social_group_id": t(group_id),                                           # (B*T, A+1) int64, -1 padded
        "action": t(action),                                                      # (B*T, A+1, 27)
        "social_group_activity": t(activity),                                     # (B*T, A+1, 27)
        "n_clips": n_clips, "n_frames": n_frames, "n_actors": n_actors,
    }


class ClipModel(nn.Module):
    """GAR_Fusion_ALL plus the clip/frame plumbing described in the module docstring."""

    def __init__(self, n_actors, n_points, gat=True, route="pointnet2", fusion="Attention_mat", modality="Multi"):
        super().__init__()
        from .model.gat_model import GAR_Fusion_ALL
        self.cfg = model_cfg(n_actors, n_points, gat, route, fusion, modality)
        self.modality = modality        # "RGB" / "LiDAR": GAR_Fusion_ALL builds that backbone alone
        self.route = route
        self.n_actors = n_actors
        self.dataset = SyntheticDataset()
        self.net = GAR_Fusion_ALL(self.cfg, self.dataset)
        self.net.GAR_model.uniform_actor_count = n_actors
        self.overlap_branches = True
        self.batch_i3d = True
        # Opt-in (bench.py --i3d-channels-last): several clips per I3D pass with the activations NDHWC between the stem and
        # the RoI crop, so that MIOpen's convolutions need no layout adapters (model/backbone.py,
        # InceptionI3d.set_channels_last).  Measured at c3: library convolutions 62.5 -> 52.9 ms, this library's BatchNorm /
        # pooling kernels +3.5 ms in that layout, step 229.4 -> ~226 ms -- but MIOpen's search over its NDHWC kernel
        # instances takes 4 min 20 s at start-up on a fresh box (NCDHW: 35-40 s), shipped find-db or not, so it is off.
        self.i3d_channels_last = False
        # Side streams of the forked and pipelined schedules, created by _make_streams
        self._rgb_stream = None         # the frozen I3D + RoIAlign pass (forked: the trainable RGB tail too)
        self._lidar_stream = None       # forked: the LiDAR branch, forward and hence backward
        self._geometry_stream = None    # the trunk's coordinate-only chain (forked: this batch's; pipelined: the next batch's)
        # Opt-in (bench.py --prefetch-geometry): input-side software pipelining.  The trunk's coordinate-only work (FPS of all
        # levels, ball queries, 3-NN weights) depends on the points alone, so a step can compute it for the NEXT batch on a side
        # stream while it runs the feature path and the backward of the current one -- as a loader would.  Every step still does
        # the geometry of one batch and the forward + backward of one batch; only the order changes.  It takes the level-1 FPS
        # (4.6 ms on 15 workgroups at one clip per rank) off the critical path.  Off by default: the headline is the plain step.
        self.geometry_prefetch = False
        self.geometry_stream_max_clouds = int(os.environ.get("MGAR_GEOMETRY_STREAM_MAX_CLOUDS", 60))   # see _forward_forked()
        # Opt-in (bench.py --prefetch-rgb): the same pipelining for the FROZEN RGB branch.  I3D + RoIAlign carry no gradient and
        # depend on the frames alone, so a step can run them for the NEXT batch on the side stream under its own BACKWARD (an
        # MFMA-bound pass beside streaming kernels) instead of beside the LiDAR forward.  Every step still runs one I3D pass; only
        # the order across the step boundary changes.  Off by default, like geometry_prefetch.
        self.rgb_prefetch = False
        self._rgb_cur = None        # RoI crops of the batch this step consumes
        self._rgb_next = None       # crops being computed for the next step (owned by the RGB stream until finish_prefetch)
        self._geo_cur = None        # geometry of the batch this step consumes (computed during the previous step)
        self._geo_next = None       # geometry being computed for the next step (owned by the geometry stream until finish_prefetch)

    # ---- RGB: one I3D pass per clip (batch 1, like the reference) ---------------------------------
    def rgb_crops(self, images, bboxes):
        """Frozen part of the RGB branch (I3D_FREEZE): I3D + RoIAlign, no autograd graph.  On the device all clips go
        through I3D in ONE pass with per-clip BatchNorm statistics (= the reference's one pass per clip, batch 1;
        fewer, larger launches: 13.5 instead of 15.0 ms per clip); elsewhere clip by clip."""
        rb = self.net.RGB_backbone
        b = images.shape[0]
        with torch.no_grad():
            if images.is_cuda and b > 1 and self.batch_i3d:
                _B, _T, _C, _H, _W = images.shape
                if self.i3d_channels_last != bool(getattr(rb.backbone_net, "channels_last", False)):
                    rb.backbone_net.set_channels_last(self.i3d_channels_last)
                rb.backbone_net.set_per_sample_stats(True)
                try:
                    crops = rb.crop_features(images.view(_B, _C, _T, _H, _W), [bboxes[i] for i in range(b)])
                finally:
                    rb.backbone_net.set_per_sample_stats(False)
                per = bboxes.shape[1]
                return [crops[i * per:(i + 1) * per] for i in range(b)]
            crops = []
            for i in range(b):
                clip = images[i:i + 1]
                _B, _T, _C, _H, _W = clip.shape
                clip = clip.view(_B, _C, _T, _H, _W)             # the reference's view (gat_model.py:1836)
                crops.append(rb.crop_features(clip, [bboxes[i]]))  # (A+1, 832, 5, 5)
        return crops

    def rgb_tokens_from_crops(self, crops, actor_counts=None):
        """Trainable tail: non-local block, pooling, embedding, optional GAT -> (B, A, 512); with actor_counts (one per
        clip) the clips' valid actors only, packed: (sum counts, 512)."""
        from .model.gat_model import fully_connected_edges
        rb = self.net.RGB_backbone
        toks = []
        for i, c in enumerate(crops):
            a = self.n_actors if actor_counts is None else actor_counts[i]
            tok = rb.embed(c[:a])                                # (A, 512)
            if rb.cfg.GAT_module:
                tok = rb.GAT_module(tok, fully_connected_edges([a], tok.device))
            toks.append(tok)
        return torch.stack(toks) if actor_counts is None else torch.cat(toks)

    def rgb_tokens(self, images, bboxes, actor_counts=None):
        return self.rgb_tokens_from_crops(self.rgb_crops(images, bboxes), actor_counts)

    # ---- LiDAR: all frames of all clips in one batch ------------------------------------------------
    def trunk_geometry(self, points, stream, whole_chain):
        """The coordinate-only part of the PointNet++ trunk issued ahead of the feature path on ``stream``: with
        ``whole_chain`` the FPS centres of the four levels, the ball queries of the folded scales and the 3-NN weights of the
        decoder; without it the level-1 FPS alone (one workgroup per cloud for ~5 ms, 6-47 % of the CUs), and the SA / FP
        modules compute the rest in line."""
        if self.route != "pointnet2":
            return None
        only_fps1 = {} if whole_chain else dict(levels=1, balls=False, neighbours=False)
        return self.net.LiDAR_backbone.model.backbone_3d.geometry(points, stream, **only_fps1)

    def lidar_tokens(self, points, bboxes3d, geometry=None, actor_counts=None):
        """-> (F, A, 512); with actor_counts (one per clip) only the valid boxes are lifted (roi_counts of the RoI heads) and
        the tokens come packed: (sum of the frames' counts, 512)."""
        f, p, _ = points.shape
        a = self.n_actors
        lb = self.net.LiDAR_backbone
        if self.route == "pointnet2":
            bidx = torch.arange(f, device=points.device, dtype=points.dtype).view(f, 1, 1).expand(f, p, 1)
            data = {"batch_size": f, "points": torch.cat([bidx, points], -1).view(f * p, 5),
                    "gt_boxes": bboxes3d[:, :a, :].contiguous(),
                    "point_batch_cnt": torch.full((f,), p, dtype=torch.int32, device=points.device)}
            if geometry is not None:
                data["trunk_geometry"] = geometry
        else:
            data = voxelize_batch(points, self.dataset)
            data["gt_boxes"] = bboxes3d[:, :a, :].contiguous()
        if actor_counts is not None:
            data["roi_counts"] = _frame_counts(actor_counts, f // len(actor_counts))
        tok = lb(data)                                           # (1, F*A, 512)
        return tok.view(f, a, -1) if actor_counts is None else tok.view(-1, tok.shape[-1])

    def finish_prefetch(self):
        """Pipelined schedule, after the step's BACKWARD (its saved index tensors are the current geometry): join the streams
        that computed the next batch's RoI crops and geometry and make those the current ones -- by copying into the current
        buffers, so that a captured HIP graph keeps reading the same addresses."""
        if self._rgb_next is not None:
            _adopt(self._rgb_stream, self._rgb_cur, self._rgb_next)
        if self._geo_next is not None:
            _adopt(self._geometry_stream, _geometry_tensors(self._geo_cur), _geometry_tensors(self._geo_next))
        self._rgb_next = self._geo_next = None

    def _make_streams(self, lidar=False, geometry=False):
        """The one place the side streams come from: each is created when a schedule first needs it."""
        if self._rgb_stream is None:
            self._rgb_stream = torch.cuda.Stream()
        if lidar and self._lidar_stream is None:
            self._lidar_stream = torch.cuda.Stream()
        if geometry and self._geometry_stream is None:
            self._geometry_stream = torch.cuda.Stream()

    def _counts(self, batch):
        """The batch's per-clip actor counts, or None when it has none or every clip is full (the uniform path, as ever)."""
        counts = batch.get("actor_counts")
        if counts is None or all(int(c) == self.n_actors for c in counts):
            return None
        return counts

    def forward(self, batch):
        """Picks one of the stream schedules; each joins its side streams into the issuing stream before the fusion net."""
        if self.modality != "Multi":
            return self._forward_single(batch)
        if not (batch["images"].is_cuda and self.overlap_branches):
            return self._forward_serial(batch)
        if (self.geometry_prefetch and self.route == "pointnet2") or self.rgb_prefetch:
            return self._forward_pipelined(batch)
        return self._forward_forked(batch)

    def _forward_serial(self, batch):
        """Everything on the current stream, in order: RGB branch, LiDAR branch, fusion net."""
        counts = self._counts(batch)
        rgb = self.rgb_tokens(batch["images"], batch["bboxes"], counts)            # (B, A, 512)
        lidar = self.lidar_tokens(batch["points"], batch["bboxes3d"], None, counts)   # (B*T, A, 512)
        return self._fuse(batch, rgb, lidar, counts)

    def _forward_single(self, batch):
        """One modality: its branch and the fusion net on the current stream, no fork; the absent side is None."""
        counts = self._counts(batch)
        rgb = lidar = None
        if self.modality == "RGB":
            rgb = self.rgb_tokens(batch["images"], batch["bboxes"], counts)
        else:
            lidar = self.lidar_tokens(batch["points"], batch["bboxes3d"], None, counts)
        return self._fuse(batch, rgb, lidar, counts)

    def _forward_forked(self, batch):
        """Both branches away from the stream the step is issued (and captured) on, which only forks and joins:

          issuing stream : records ``inputs_ready``; ... waits for geometry, RGB, LiDAR stream (in that order); fusion net
          RGB stream     : waits for inputs_ready; frozen I3D + RoIAlign, then the trainable RGB tail        (issued first)
          geometry stream: waits for inputs_ready; the trunk's whole coordinate-only chain                  (issued second;
                           PointNet++ route with at most ``geometry_stream_max_clouds`` clouds only)
          LiDAR stream   : waits for inputs_ready; the LiDAR branch, whose SA / FP modules wait for the geometry stream's
                           per-level events where that stream is in use and compute the geometry in line otherwise

        The backward of each branch runs on the stream of its forward.  The measurements behind the issue order, the RGB tail
        on the RGB stream and the 60-cloud limit of the geometry stream: DESIGN.md section 4a."""
        points = batch["points"]
        counts = self._counts(batch)
        use_geometry_stream = self.route == "pointnet2" and points.shape[0] <= self.geometry_stream_max_clouds
        self._make_streams(lidar=True, geometry=use_geometry_stream)
        main = torch.cuda.current_stream()
        inputs_ready = main.record_event()
        self._rgb_stream.wait_event(inputs_ready)
        with torch.cuda.stream(self._rgb_stream):
            crops = self.rgb_crops(batch["images"], batch["bboxes"])
            rgb = self.rgb_tokens_from_crops(crops, counts)
        geometry = None
        if use_geometry_stream:
            self._geometry_stream.wait_event(inputs_ready)
            geometry = self.trunk_geometry(points, self._geometry_stream, whole_chain=True)
        self._lidar_stream.wait_event(inputs_ready)
        with torch.cuda.stream(self._lidar_stream):
            lidar = self.lidar_tokens(points, batch["bboxes3d"], geometry, counts)
        if use_geometry_stream:
            main.wait_stream(self._geometry_stream)
        main.wait_stream(self._rgb_stream)
        main.wait_stream(self._lidar_stream)
        if not torch.cuda.is_current_stream_capturing():   # inside a graph the pool is private and replays are serial
            for c in crops:
                c.record_stream(main)
            lidar.record_stream(main)
            rgb.record_stream(main)
        return self._fuse(batch, rgb, lidar, counts)

    def _forward_pipelined(self, batch):
        """Input-side software pipelining (``geometry_prefetch`` and / or ``rgb_prefetch``): the LiDAR branch, the trainable
        RGB tail and the fusion net on the issuing stream, the input-only work of the NEXT batch on side streams.

          issuing stream : records ``inputs_ready``; [first step only: what was not prefetched, in line]; without
                           geometry_prefetch the level-1 FPS ahead of everything else (a single launch that leaves most of the
                           chip idle); LiDAR branch; waits for the RGB stream (without rgb_prefetch); RGB tail; fusion net
          geometry stream: (geometry_prefetch) waits for inputs_ready; the whole coordinate-only chain of the next batch
          RGB stream     : without rgb_prefetch: waits for inputs_ready; this batch's frozen I3D + RoIAlign
                           with rgb_prefetch: waits for the end of the forward; the next batch's frozen pass,
                           which then runs under this step's objective and backward

        ``finish_prefetch`` joins what ran for the next batch, after the backward."""
        geometry_prefetch = self.geometry_prefetch and self.route == "pointnet2"
        counts = self._counts(batch)
        self._make_streams(geometry=geometry_prefetch)
        main = torch.cuda.current_stream()
        inputs_ready = main.record_event()
        if geometry_prefetch:
            if self._geo_cur is None:      # first step: nothing was prefetched -- compute it in line, once
                self._geo_cur = _without_events(self.trunk_geometry(batch["points"], main, whole_chain=True))
            geometry = self._geo_cur
            # the NEXT batch's geometry (the caller passes its points; the benchmark's batches are all the same tensor)
            self._geometry_stream.wait_event(inputs_ready)
            self._geo_next = self.trunk_geometry(batch.get("next_points", batch["points"]), self._geometry_stream, whole_chain=True)
        else:
            geometry = self.trunk_geometry(batch["points"], main, whole_chain=False)
        if self.rgb_prefetch:
            if self._rgb_cur is None:      # first step: nothing was prefetched -- compute it in line, once
                self._rgb_cur = [c.clone() for c in self.rgb_crops(batch["images"], batch["bboxes"])]
            crops = self._rgb_cur
        else:
            self._rgb_stream.wait_event(inputs_ready)
            with torch.cuda.stream(self._rgb_stream):
                crops = self.rgb_crops(batch["images"], batch["bboxes"])
        lidar = self.lidar_tokens(batch["points"], batch["bboxes3d"], geometry, counts)   # (B*T, A, 512)
        if not self.rgb_prefetch:
            main.wait_stream(self._rgb_stream)
            if not torch.cuda.is_current_stream_capturing():   # inside a graph the pool is private and replays are serial
                for c in crops:
                    c.record_stream(main)
        rgb = self.rgb_tokens_from_crops(crops, counts)                           # (B, A, 512)
        out = self._fuse(batch, rgb, lidar, counts)
        if self.rgb_prefetch:
            # the NEXT batch's frozen RGB pass (the caller passes its frames; the benchmark's batches are all the same tensor),
            # issued where the forward ends
            self._rgb_stream.wait_event(main.record_event())
            with torch.cuda.stream(self._rgb_stream):
                self._rgb_next = self.rgb_crops(batch.get("next_images", batch["images"]), batch.get("next_bboxes", batch["bboxes"]))
        return out

    def _fuse(self, batch, rgb, lidar, counts=None):
        if counts is not None:
            return self._fuse_ragged(batch, rgb, lidar, counts)
        b, t, a = batch["n_clips"], batch["n_frames"], self.n_actors
        if rgb is not None:
            rgb = rgb[:, None].expand(b, t, a, rgb.shape[-1]).reshape(b * t, a, -1)  # every frame-scene of a clip
        # MNP = A + 1; a single-modality model passes None for the absent side
        pad = lambda x: None if x is None else torch.cat([x, x.new_zeros(x.shape[0], 1, x.shape[2])], 1).float()  # noqa: E731
        bb2 = batch["bboxes"][:, None].expand(b, t, a + 1, 4).reshape(b * t, a + 1, 4)
        # The fusion net works on (A, 512) tokens per scene: launch-bound, not bandwidth-bound.  It runs in fp32 on every
        # configuration (under the bf16 configurations the token producers above are bf16; the tokens are widened here).
        with torch.autocast(device_type=bb2.device.type, enabled=False):
            return self.net.GAR_model(pad(rgb), pad(lidar), bb2, batch["bboxes3d"], None, batch["person_id"])

    def _fuse_ragged(self, batch, rgb, lidar, counts):
        """rgb: the clips' tokens packed (sum of the clips' counts, 512); lidar: the frame-scenes' tokens packed.  Every
        frame-scene of a clip takes its clip's RGB rows and key-frame boxes through a cached index; the fusion net gets
        packed rows and the frames' counts, so nothing is padded and gathered again."""
        from .scene_ops import scene_layout
        t, mnp = batch["n_frames"], self.n_actors + 1
        frames = _frame_counts(counts, t)
        dev = batch["bboxes"].device
        tok_rows, box_rows = _clip_rows(counts, t, mnp, dev)
        slot = scene_layout(frames, mnp, dev).row_slot
        gar = self.net.GAR_model
        with torch.autocast(device_type=dev.type, enabled=False):
            R = None if rgb is None else rgb.float()[tok_rows]           # a single-modality model: the absent side is None
            L = None if lidar is None else lidar.float()
            bb = batch["bboxes"].reshape(-1, 4)[box_rows]
            b3 = batch["bboxes3d"].reshape(-1, batch["bboxes3d"].shape[-1])[slot]
            if gar._scene_counts_ok(frames):
                return gar.forward_packed(R, L, bb, b3[:, :3], frames, mnp)
            # scene by scene, as the reference loops: the same rows in the zero-padded tensors of its interface
            s = len(frames)
            pad = lambda x: None if x is None else x.new_zeros(s * mnp, x.shape[1]).index_copy(0, slot, x).view(s, mnp, -1)  # noqa: E731
            return gar.forward_per_scene(pad(R), pad(L), pad(bb), batch["bboxes3d"], None, batch["person_id"])


_CLIP_ROWS = {}


def _frame_counts(actor_counts, n_frames):
    """Per-clip counts -> one count per frame-scene (every frame of a clip has its clip's count)."""
    return [int(c) for c in actor_counts for _ in range(n_frames)]


def _clip_rows(actor_counts, n_frames, mnp, device):
    """For every packed frame-scene row: its row in the clips' packed tokens, and its row in the clips' (B * MNP) key-frame
    boxes.  Built on the host once per (counts, frames, MNP, device)."""
    key = (tuple(actor_counts), n_frames, mnp, str(device))
    hit = _CLIP_ROWS.get(key)
    if hit is None:
        tok, box, off = [], [], 0
        for c, a in enumerate(actor_counts):
            for _ in range(n_frames):
                tok += range(off, off + a)
                box += range(c * mnp, c * mnp + a)
            off += a
        hit = (torch.tensor(tok, dtype=torch.int64, device=device), torch.tensor(box, dtype=torch.int64, device=device))
        if len(_CLIP_ROWS) < 64:
            _CLIP_ROWS[key] = hit
    return hit


def _adopt(stream, current, prefetched):
    """Join ``stream`` into the current one and copy the tensors it produced over the current ones."""
    main = torch.cuda.current_stream()
    main.wait_stream(stream)
    assert len(current) == len(prefetched)
    capturing = torch.cuda.is_current_stream_capturing()
    for cur, nxt in zip(current, prefetched):
        if not capturing:
            nxt.record_stream(main)
        cur.copy_(nxt)


def _geometry_tensors(geo):
    out = list(geo.centres)
    for idx in geo.ball_idx:
        if isinstance(idx, dict):
            out += [idx[k] for k in sorted(idx)]
        elif torch.is_tensor(idx):
            out.append(idx)
    for i in sorted(geo.nn):
        out += list(geo.nn[i])
    return out


def _without_events(geo):
    """The same TrunkGeometry with no stream events: its producer has been joined already (or ran on the consumer's stream)."""
    geo.centre_events = [None] * len(geo.centre_events)
    geo.idx_events = [None] * len(geo.idx_events)
    geo.nn_events = {i: None for i in geo.nn_events}
    return geo


def voxelize_batch(points, dataset, max_points=5, max_voxels=40000):
    """(F, P, 4) -> the dict MeanVFE / the sparse trunk consume (voxels, counts, coords [b, z, y, x]): the reference's host
    voxeliser call (pcdet/datasets/processor/data_processor.py:15-60, 132-152) for all clouds of the batch at once, on the
    tensors' device, with the same semantics (first-appearance voxel order, first max_points points, max_voxels cap)."""
    from .pcdet.datasets.processor.data_processor import points_to_voxels_batch
    return points_to_voxels_batch(points, dataset.point_cloud_range, dataset.voxel_size, max_points, max_voxels)


def voxel_route_capturable():
    """Whether the voxel route can be recorded into a HIP graph: its voxeliser has data-dependent sizes (torch.unique ->
    host sync), so not yet."""
    from .pcdet.datasets.processor import data_processor
    return bool(getattr(data_processor, "FIXED_CAPACITY", False))


def synthetic_loss(outputs):
    """Scalar over all 16 outputs so that every trainable parameter receives a gradient (round-1 placeholder objective;
    kept for tests that need a label-free scalar)."""
    return sum((o.float() ** 2).mean() for o in outputs)


def reference_loss(outputs, batch):
    """The reference's training objective (train_func.py:166-256, Loss = "L_total" as train_func.py:553 selects it: weighted
    adjacency BCE + individual pose CE / interaction BCE + social-group pose / interaction BCE) on synthetic annotations,
    evaluated on the device without a Python loop over scenes (losses.mgar_losses_uniform).  Every frame-scene is one sample;
    the per-sample terms are summed over the scenes, which is what the reference accumulates at its BATCH_SIZE 1
    (train_func.py:260-269).  As in the reference, the cardinality head is not part of L_total and receives no gradient."""
    from . import losses
    counts = batch.get("actor_counts")
    if counts is not None and any(int(c) != batch["n_actors"] for c in counts):
        return losses.mgar_losses_ragged(outputs, batch["social_group_id"], batch["action"], batch["social_group_activity"],
                                         _frame_counts(batch["actor_counts"], batch["n_frames"]), Loss="L_total",
                                         reference_semantics=False)["L_total"]
    return losses.mgar_losses_uniform(outputs, batch["social_group_id"], batch["action"], batch["social_group_activity"],
                                      batch["n_actors"], Loss="L_total", reference_semantics=False)["L_total"]


class _GraphStep:
    """What TrainStep and ForwardStep share: warm-up, capture into a HIP graph (torch.cuda.CUDAGraph) and replay on a static
    batch.  A subclass provides ``run_eager(batch)`` and decides what it records."""
    graph = None
    _static_batch = None

    def _warm_up(self, batch, warmup):
        """``batch``'s tensors become the static inputs (later batches are copied into them); `warmup` eager steps run
        first on a side stream, as graph capture requires."""
        assert self.graph is None and batch["images"].is_cuda
        self._static_batch = batch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.run_eager(batch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _record(self, fn):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        self.graph = graph
        return out

    def _replay(self, batch):
        if batch is not self._static_batch:
            for k, v in batch.items():
                if torch.is_tensor(v):
                    self._static_batch[k].copy_(v)
        self.graph.replay()


class TrainStep(_GraphStep):
    """model + Adam + data parallelism; ``run(batch)`` = forward, loss, backward, (gradient all-reduce,) optimizer step.

    ddp=True wraps the model in DistributedDataParallel (bucketed all-reduce overlapped with backward).
    ``capture(batch)`` records forward + backward of one step into a HIP graph (torch.cuda.CUDAGraph): the ~1 900-
    4 700 launches of a step are replayed without the host, which is what bounds a rank that holds a single clip.
    In graph mode the data-parallel exchange is ONE all-reduce of the flattened gradients after the replay
    (no DDP wrapper: its hooks cannot live inside a captured backward), then Adam."""

    def __init__(self, n_actors, n_points, device, gat=True, route="pointnet2", ddp=False, lr=1e-3, seed=2023,
                 manual_allreduce=False, loss="reference", fusion="Attention_mat", modality="Multi"):
        assert loss in ("reference", "synthetic")
        self.loss_kind = loss
        torch.manual_seed(seed)  # the reference seeds 2023 (train_func.py:45-47)
        self.model = ClipModel(n_actors, n_points, gat, route, fusion, modality).to(device)
        self.model.train()
        self.module = self.model
        self.manual_allreduce = bool(manual_allreduce)
        # The reference objective is a SUM over the scenes of the batch (what train_func.py:260-269 accumulates over its
        # micro-steps), so the gradient of the GLOBAL batch is the SUM of the ranks' gradients: all-reduce(SUM), no division --
        # an N-rank step is then the same update as the one-rank step on the same global batch.  The label-free
        # synthetic objective is a mean, whose global gradient is the ranks' average.
        self.grad_average = (loss == "synthetic")
        self._ddp_wrapped = bool(ddp and not manual_allreduce)
        if ddp and not manual_allreduce:
            from torch.nn.parallel import DistributedDataParallel as DDP
            dev_ids = [device.index] if device.type == "cuda" else None
            # the reference objective leaves the cardinality head (and, on the voxel route, conv_out / shared_fc) without a
            # gradient on every rank: the reducer has to be told, or the buckets holding them are never exchanged
            self.model = DDP(self.model, device_ids=dev_ids, find_unused_parameters=(loss == "reference"),
                             gradient_as_bucket_view=True, bucket_cap_mb=64)
        if ddp and manual_allreduce:
            self._sync_from_rank0()
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        # train_func.py:552 Adam(lr=1e-3); on the device the fused implementation (a handful of launches instead of ~30)
        self.opt = torch.optim.Adam(self.params, lr=lr, fused=(device.type == "cuda") or None)
        self._loss = None

    # ---- eager step ------------------------------------------------------------------------------
    def _forward_backward(self, batch):
        self.opt.zero_grad(set_to_none=True)
        out = self.model(batch)
        loss = self._loss_of(out, batch)
        if self._ddp_wrapped and not self.grad_average:
            # DistributedDataParallel averages the ranks' gradients; a summed objective wants their sum
            import torch.distributed as dist
            (loss * dist.get_world_size()).backward()
        else:
            loss.backward()
        self.module.finish_prefetch()
        return loss.detach()

    def _loss_of(self, out, batch):
        return reference_loss(out, batch) if self.loss_kind == "reference" else synthetic_loss(out)

    def _sync_from_rank0(self):
        """Flat-all-reduce data parallelism: every rank starts from rank 0's parameters and buffers (DistributedDataParallel
        does this itself).  BatchNorm running statistics then evolve per rank -- they are never exchanged, as under the
        reference's nn.DataParallel, whose replicas' buffer updates are discarded except replica 0's (train_func.py:512)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        with torch.no_grad():
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                dist.broadcast(t, src=0)

    def _exchange_gradients(self):
        """One all-reduce(SUM) over all gradients, flattened (~119 MB fp32 per step); divided by the
        world size only for an averaged objective (see ``grad_average``)."""
        if not self.manual_allreduce:
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        # parameters outside the objective (the cardinality head under L_total; conv_out / shared_fc of the voxel route, unused
        # downstream as in the reference) have no gradient on ANY rank: the layout below is the same everywhere.  A parameter
        # that received a gradient on some ranks only would desynchronise the collective, so the set is pinned at the first step.
        have = tuple(p.grad is not None for p in self.params)
        if getattr(self, "_grad_layout", None) is None:
            self._grad_layout = have
        assert have == self._grad_layout, "the set of parameters with gradients changed between steps"
        grads = [p.grad for p in self.params if p.grad is not None]
        flat = torch._utils._flatten_dense_tensors(grads)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if self.grad_average:
            flat.div_(dist.get_world_size())
        for g, f in zip(grads, torch._utils._unflatten_dense_tensors(flat, grads)):
            g.copy_(f)

    def run_eager(self, batch):
        loss = self._forward_backward(batch)
        self._exchange_gradients()
        self.opt.step()
        return loss

    # ---- HIP-graph step ---------------------------------------------------------------------------
    def capture(self, batch, warmup=2):
        """Record forward + backward on ``batch``, after `warmup` eager steps."""
        assert not hasattr(self.model, "module") or self.model is self.module, "capture() needs manual_allreduce, not DDP"
        self._warm_up(batch, warmup)
        self.opt.zero_grad(set_to_none=True)

        def forward_backward():
            loss = self._loss_of(self.model(batch), batch)
            loss.backward()
            self.module.finish_prefetch()
            return loss.detach()
        self._loss = self._record(forward_backward)
        self._graph_grads = [p.grad for p in self.params]   # the buffers every replay writes (graph-private pool)
        return self

    def run(self, batch):
        if self.graph is None:
            return self.run_eager(batch)
        self._replay(batch)
        for p, g in zip(self.params, self._graph_grads):      # an eager step in between re-points .grad elsewhere
            p.grad = g
        self._exchange_gradients()
        self.opt.step()
        return self._loss


class ForwardStep(_GraphStep):
    """Train-mode forward of the clip model (batch-statistics BatchNorm, dropout active) without autograd: the workload of
    BASELINE configs c2 / c5.  precision="bf16": feature payloads and GEMMs / convolutions in bf16 -- the hand-written
    kernels take bf16 payloads directly (include/mgar_ops.h, `_bf16` entry points: fp32 arithmetic inside, fp32 BatchNorm
    statistics), library GEMMs / convolutions run under torch.autocast(bfloat16) -- while coordinates, distances, indices
    and the per-scene fusion net stay fp32 / int32 (SURVEY.md section 8 header), so every index tensor is bit-identical to
    the fp32 run.  Same interface as TrainStep (capture / run / run_eager, .module, .graph)."""

    def __init__(self, n_actors, n_points, device, gat=True, route="pointnet2", precision="fp32", seed=2023,
                 fusion="Attention_mat", modality="Multi"):
        assert precision in ("fp32", "bf16")
        torch.manual_seed(seed)
        self.model = ClipModel(n_actors, n_points, gat, route, fusion, modality).to(device)
        self.model.train()
        self.module = self.model
        self.precision = precision
        self.device = device
        if precision == "bf16" and modality != "LiDAR":
            # the frozen I3D's convolution weights are converted once (autocast would re-cast them every step);
            # BatchNorm vectors and every trainable parameter stay fp32
            for m in self.model.net.RGB_backbone.backbone_net.modules():
                if isinstance(m, nn.Conv3d):
                    m.weight.data = m.weight.data.to(torch.bfloat16)
        self._out = None

    def _forward(self, batch):
        with torch.no_grad(), torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=self.precision == "bf16"):
            return self.model(batch)

    def run_eager(self, batch):
        return self._forward(batch)

    def capture(self, batch, warmup=2):
        self._warm_up(batch, warmup)
        self._out = self._record(lambda: self._forward(batch))
        return self

    def run(self, batch):
        if self.graph is None:
            return self._forward(batch)
        self._replay(batch)
        return self._out


Inference = namedtuple("Inference", "outputs group_id")
Inference.__doc__ = """outputs: the 16 zero-padded tensors of GAR_Fusion_Net3.forward; group_id (S, MNP) int32: the social group
the model predicts for every actor -- the smallest j whose thresholded adjacency a_ij >= 0.5, with a_ii = 1 -- and -1 in the
padding slots."""


def predicted_group_ids(gar, a_list, counts):
    """The group ids of GAR_Fusion_Net3._predicted_groups for every scene of a returned A_list (S, MNP, MNP), counts[s] valid
    actors in scene s (host ints) -> (S, MNP) int32, -1 in the padding.  Device ops only."""
    s, mnp = a_list.shape[0], a_list.shape[1]
    out = torch.full((s, mnp), -1, dtype=torch.int32, device=a_list.device)
    for i, n in enumerate(counts):
        out[i, :n] = gar._predicted_groups(a_list[i, :n, :n]).to(torch.int32)
    return out


class InferStep(_GraphStep):
    """Eval-mode forward of the clip model: the whole ClipModel in .eval() (running-statistics BatchNorm folded into the
    kernels' stores, no dropout) under torch.no_grad(), the inference route of every module.  Same interface and precision rule
    as ForwardStep (capture / run / run_eager, .module, .graph; precision="bf16" converts the frozen I3D's convolution
    weights once); ``run`` returns Inference(outputs, group_id).  The group ids come from the fused tail kernel
    (scene_tail_ops) where the fusion net takes it and from _predicted_groups on the returned adjacency otherwise.  No
    BatchNorm buffer is written.  The voxel route is eager only while voxel_route_capturable() says so: capture() raises."""

    def __init__(self, n_actors, n_points, device, gat=True, route="pointnet2", precision="fp32", seed=2023,
                 fusion="Attention_mat", modality="Multi"):
        assert precision in ("fp32", "bf16")
        torch.manual_seed(seed)
        self.model = ClipModel(n_actors, n_points, gat, route, fusion, modality).to(device)
        self.model.eval()
        self.module = self.model
        self.precision = precision
        self.device = device
        self.route = route
        if precision == "bf16" and modality != "LiDAR":
            for m in self.model.net.RGB_backbone.backbone_net.modules():
                if isinstance(m, nn.Conv3d):
                    m.weight.data = m.weight.data.to(torch.bfloat16)
        self._out = None

    def _scene_counts(self, batch):
        counts = batch.get("actor_counts")
        if counts is None:
            return [self.model.n_actors] * (batch["n_clips"] * batch["n_frames"])
        return _frame_counts(counts, batch["n_frames"])

    def _forward(self, batch):
        gar = self.model.net.GAR_model
        with torch.no_grad(), torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=self.precision == "bf16"):
            gar._tail_group_id = None
            outputs = self.model(batch)
            group_id = gar._tail_group_id
            if group_id is None:
                group_id = predicted_group_ids(gar, outputs[0].float(), self._scene_counts(batch))
        return Inference(tuple(outputs), group_id)

    def run_eager(self, batch):
        return self._forward(batch)

    def capture(self, batch, warmup=2):
        if self.route == "voxel" and self.model.modality != "RGB" and not voxel_route_capturable():
            raise RuntimeError("InferStep.capture: the voxel route is eager only (voxel_route_capturable())")
        self._warm_up(batch, warmup)
        self._out = self._record(lambda: self._forward(batch))
        return self

    def run(self, batch):
        if self.graph is None:
            return self._forward(batch)
        self._replay(batch)
        return self._out


def trainable_parameter_count(module):
    return sum(p.numel() for p in module.parameters() if p.requires_grad)
