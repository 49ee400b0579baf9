"""SECOND-KITTI forward + NMS on one MI355X (BASELINE.json configs[2]): batched HIP voxelise -> MeanVFE -> sparse 3D
backbone (rulebooks + mask-ordered MFMA implicit GEMM, fused BN/ReLU epilogues) -> .dense() / HeightCompression -> folded
BEV backbone + merged heads -> HIP anchor post-processing -> batched rotated NMS.

Topology from tools/cfgs/kitti_models/second.yaml: VoxelBackBone8x (pcdet/models/backbones_3d/spconv_backbone.py:68-163),
HeightCompression (pcdet/models/backbones_2d/map_to_bev/height_compression.py:10-26), BaseBEVBackbone with LAYER_NUMS [5, 5],
LAYER_STRIDES [1, 2], NUM_FILTERS [128, 256], UPSAMPLE_STRIDES [1, 2], NUM_UPSAMPLE_FILTERS [256, 256]
(base_bev_backbone.py:6-112), AnchorHeadSingle with the three KITTI anchor classes x 2 rotations.  Random-init weights;
everything downstream of the heads is shared with pointpillar.PointPillarKITTI."""
import numpy as np
import torch
import torch.nn as nn

from . import pillar_ops, spconv, synth
from .bev_backbone import FoldedBEVBackbone
from .bev_train import _check_deblock, _check_wgrad
from .pcdet.models.backbones_3d import spconv_backbone
from .pcdet.utils.cfg import AttrDict
from .pointpillar import (KITTI_ANCHORS, KITTI_CLASS_NAMES, KITTI_THRESHOLDS, PointPillarKITTI, generate_anchors,
                          make_bev_backbone)
from .voxelizer import BatchVoxelizer, grid_size_of

# second.yaml DENSE_HEAD: what the training loss reads (anchors on the stride-8 map, target assigner, loss) — SECONDKitti.rpn_loss
DENSE_HEAD_CFG = dict(
    NAME="AnchorHeadSingle", USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
    ANCHOR_GENERATOR_CONFIG=[dict(class_name=n, anchor_sizes=[s], anchor_rotations=r, anchor_bottom_heights=[h], align_center=False,
                                  feature_map_stride=8, matched_threshold=t[0], unmatched_threshold=t[1])
                             for n, (s, r, h), t in zip(KITTI_CLASS_NAMES, KITTI_ANCHORS, KITTI_THRESHOLDS)],
    TARGET_ASSIGNER_CONFIG=dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False,
                                MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"),
    LOSS_CONFIG=dict(LOSS_WEIGHTS={"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2, "code_weights": [1.0] * 7}))
SPARSE_OPTIONS = ("stock", "fused")


def _check_sparse(sparse, who):
    if sparse not in SPARSE_OPTIONS:
        raise pillar_ops._lib.LidarHipError(f"{who}: sparse must be one of {SPARSE_OPTIONS}, got {sparse!r}")
    return sparse


class SECONDKitti(PointPillarKITTI):
    def __init__(self, batch_size=16, max_voxels=16000, n_max=20000, device="cuda", score_thresh=0.1, nms_thresh=0.01,
                 nms_pre=4096, nms_post=500):
        nn.Module.__init__(self)
        self.B, self.n_max = batch_size, n_max
        self.pc_range, self.voxel_size = synth.SEC_RANGE, synth.SEC_VOXEL
        self.grid = [int(v) for v in grid_size_of(self.voxel_size, self.pc_range)]          # [1408, 1600, 40]
        self.voxelizer = BatchVoxelizer(self.voxel_size, self.pc_range, 5, max_voxels, 4)
        self.backbone3d = spconv_backbone.VoxelBackBone8x(AttrDict(), 4, self.grid)
        self.blocks, self.deblocks = make_bev_backbone(cin=256, layer_nums=(5, 5), strides=(1, 2), filters=(128, 256),
                                                       up_strides=(1, 2), up_filters=(256, 256))
        self.num_class, self.num_anchor_per_loc, self.num_dir_bins = 3, 6, 2
        self.conv_cls = nn.Conv2d(512, self.num_anchor_per_loc * self.num_class, 1)
        self.conv_box = nn.Conv2d(512, self.num_anchor_per_loc * 7, 1)
        self.conv_dir_cls = nn.Conv2d(512, self.num_anchor_per_loc * self.num_dir_bins, 1)
        self.dir_offset, self.dir_limit_offset = 0.78539, 0.0
        self.score_thresh, self.nms_thresh, self.nms_pre, self.nms_post = score_thresh, nms_thresh, nms_pre, nms_post
        self.channels_last = self.fold_bn = True
        self.to(device).eval()
        for mod in (self.blocks, self.deblocks, self.conv_cls, self.conv_box, self.conv_dir_cls):
            mod.to(memory_format=torch.channels_last)       # 2D part only (the sparse weights are 5-D)
        self.anchors = generate_anchors(self.pc_range, (self.grid[1] // 8, self.grid[0] // 8), device)
        self._vox_out = self.voxelizer.alloc_outputs(batch_size, device)
        self._folded = self._bev = None

    # ---- stages --------------------------------------------------------------------------------
    def voxelize_vfe(self, points, point_offsets, host_offsets=None):
        vox = self.voxelizer(points, point_offsets, self.n_max, compact=True, out=self._vox_out, resident=self.resident_voxels,
                             host_offsets=host_offsets)
        total = int(vox["voxel_offsets"][self.B])               # the sparse stack needs exact row counts (one read-back)
        feats = pillar_ops.mean_vfe(vox["voxels"][:total], vox["voxel_num_points"][:total])
        return feats, vox["voxel_coords"][:total]

    def sparse_backbone(self, feats, coords):
        bd = self.backbone3d({"voxel_features": feats, "voxel_coords": coords, "batch_size": self.B})
        return bd["encoded_spconv_tensor"].dense_bev()          # (B, 128 * 2, 200, 176), channels-last, one pass

    def backbone_head(self, canvas):
        return (self._bev_folded().merged(canvas),)

    @torch.no_grad()
    def forward(self, points, point_offsets, host_offsets=None):
        feats, coords = self.voxelize_vfe(points, point_offsets, host_offsets)
        canvas = self.sparse_backbone(feats, coords)
        return self.post_process(*self.backbone_head(canvas))

    # ---- training ------------------------------------------------------------------------------
    def _loss_head(self):
        if self.__dict__.get("_rpn_loss_head") is None:
            from .pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
            cfg = AttrDict({k: AttrDict(v) if isinstance(v, dict) else v for k, v in DENSE_HEAD_CFG.items()})
            with torch.cuda.device(self.anchors.device):
                self.__dict__["_rpn_loss_head"] = AnchorHeadTemplate(cfg, self.num_class, KITTI_CLASS_NAMES, np.array(self.grid),
                                                                     self.pc_range, False)
        return self.__dict__["_rpn_loss_head"]

    def train_loss(self, points, point_offsets, gt_boxes, host_offsets=None, backbone="stock", sparse="stock", wgrad="library",
                   deblock="library"):
        """One training forward of SECOND-KITTI on this package's kernels: voxelise into fresh buffers (no gradient), MeanVFE,
        VoxelBackBone8x in grad mode (train-mode BatchNorm1d on batch statistics; running statistics are updated), the
        differentiable HeightCompression (SparseConvTensor.dense_bev), the BEV backbone and heads (train-mode BatchNorm2d) and
        rpn_loss (second.yaml's head: stride-8 anchors).  -> (cls_loss, loc_loss, dir_loss), differentiable with respect to every
        parameter.  gt_boxes (B, M, 8) [box | class id].
        sparse: "stock" (torch BatchNorm1d / ReLU modules between the sparse convolutions) or "fused" (spconv.fused_bn_train: every
        BatchNorm1d -> ReLU pair as one fused call forward and one backward).
        backbone: "stock" (backbone_head_stock: torch modules) or "fused" (backbone_head_train); wgrad ("library" or "wino") and
        deblock ("library" or "gemm") are backbone_head_train's options and have no effect on the "stock" backbone.
        Host synchronisations: the voxel total is read back once (the sparse stack needs exact row counts), and the exact rulebook
        path reads one output-site count back per strided convolution (4 in VoxelBackBone8x).  The step is therefore not
        graph-capturable."""
        head, _, _ = self.train_trunk(points, point_offsets, host_offsets, backbone, sparse, wgrad, deblock, "SECONDKitti.train_loss")
        return self.rpn_loss(head, gt_boxes)

    def train_trunk(self, points, point_offsets, host_offsets=None, backbone="stock", sparse="stock", wgrad="library",
                    deblock="library", who="SECONDKitti.train_trunk"):
        """train_loss() up to the heads -> (head outputs (cls, box, dirs), the sparse backbone's multi-scale tensors, the BEV map):
        what a second stage (PVRCNNKitti.train_loss) reads beside the RPN loss.  Arguments as train_loss()."""
        err = pillar_ops._lib.LidarHipError
        if not self.training:
            raise err(f"{who} needs train mode (call .train() first)")
        if backbone not in ("stock", "fused"):
            raise err(f"{who}: backbone must be 'stock' or 'fused', got {backbone!r}")
        _check_sparse(sparse, who)
        _check_wgrad(wgrad, who)
        _check_deblock(deblock, who)
        with torch.no_grad():   # fresh voxel buffers: the first sparse layer's backward reads the features after the next step may have voxelised
            vox = self.voxelizer(points, point_offsets, self.n_max, compact=True, host_offsets=host_offsets)
            total = int(vox["voxel_offsets"][self.B])           # one read-back: exact row counts for the sparse stack
            feats = pillar_ops.mean_vfe(vox["voxels"][:total], vox["voxel_num_points"][:total])
        coords = vox["voxel_coords"][:total]
        with spconv.fused_bn_train(sparse == "fused"):
            bd = self.backbone3d({"voxel_features": feats, "voxel_coords": coords, "batch_size": self.B})
        canvas = bd["encoded_spconv_tensor"].dense_bev()
        if backbone != "fused":
            head = self.backbone_head_stock(canvas)
        else:
            head = self.backbone_head_train(canvas, wgrad, deblock)
        return head, bd["multi_scale_3d_features"], canvas
