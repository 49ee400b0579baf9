"""PV-RCNN-KITTI forward on one MI355X (BASELINE.json configs[3], bs 8): the SECOND trunk plus the point branch and the RoI head.

Topology from tools/cfgs/kitti_models/pv_rcnn.yaml (test mode), written from its shapes:
  voxelise -> MeanVFE -> VoxelBackBone8x (keeps x_conv1..4) -> HeightCompression -> BaseBEVBackbone [5, 5] -> AnchorHeadSingle
  -> proposals: class-agnostic rotated NMS on the raw class logits, pre 1024 / thr 0.7 / post 100 (roi_head_template.py:45-99)
  -> VoxelSetAbstraction (pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:119-240): 2048 keypoints per frame by
     furthest-point sampling of the raw points; per keypoint: bilinear BEV features (256) + StackSAModuleMSG over the raw points
     (radii 0.4/0.8, 16/16 samples, 4 -> 16 -> 16 twice) and over the voxel centres of x_conv1..4 (:120-144 of the yaml);
     640 -> 128 fusion (Linear + BN + ReLU)
  -> PointHeadSimple (dense_heads/point_head_simple.py:60-90): 640 -> 256 -> 256 -> 1, sigmoid = keypoint weight
  -> PVRCNNHead (roi_heads/pvrcnn_head.py:73-177): 6^3 grid points per RoI, StackSAModuleMSG over the weighted keypoints
     (radii 0.8/1.6, 16/16 samples, 131 -> 64 -> 64 twice), shared FC 27648 -> 256 -> 256, class and box branches, box decode
     relative to the RoI (roi_head_template.py:235-263)
  -> final class-agnostic NMS: sigmoid(score) >= 0.1, thr 0.1, post 500 (detector3d_template.py:236-262).
Hot-path ops are this repo's HIP kernels (voxelise, sparse conv, FPS, ball query, grouping, batched NMS, anchor decode); MLPs are
stock torch.  Batched where the reference loops over samples in Python: one FPS launch for all frames of equal size, per-level
point counts by bincount, ONE batched NMS for the proposals of all frames and one for the final boxes.  Random-init weights.
"""
import numpy as np
import torch
import torch.nn as nn

from . import anchor_post, point_head, roi_loss
from .ext import iou3d_nms_cuda
from .pcdet.ops.pointnet2 import _common as pn_common
from .pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pn_batch
from .pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pn_stack_modules
from .pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pn_stack
from .pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from .pcdet.utils import common_utils
from .pcdet.utils.cfg import AttrDict
from .second import SECONDKitti

# pv_rcnn.yaml:119-144: source -> (downsample factor, radii, nsamples, MLP widths behind the input width)
VSA_SOURCES = {
    "x_conv1": (1, [0.4, 0.8], [16, 16], [[16, 16], [16, 16]], 16),
    "x_conv2": (2, [0.8, 1.2], [16, 32], [[32, 32], [32, 32]], 32),
    "x_conv3": (4, [1.2, 2.4], [16, 32], [[64, 64], [64, 64]], 64),
    "x_conv4": (8, [2.4, 4.8], [16, 32], [[64, 64], [64, 64]], 64),
}

# pv_rcnn.yaml:190-202: ROI_HEAD.TARGET_CONFIG
TARGET_CONFIG = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
                     CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
# pv_rcnn.yaml:204-218: ROI_HEAD.LOSS_CONFIG
LOSS_CONFIG = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                   LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0, code_weights=[1.0] * 7))
# pv_rcnn.yaml:146-157: POINT_HEAD (class-agnostic: one class)
POINT_HEAD_CONFIG = dict(TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
                         LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0)))


def bilinear_bev(bev_nhwc, x, y):
    """bev_nhwc (B, H, W, C), x / y (B, M) in feature-map cells -> (B, M, C); the reference's bilinear_interpolate_torch
    (voxel_set_abstraction.py:9-39) for all frames at once: clamped corner indices, UNclamped weights."""
    B, H, W, C = bev_nhwc.shape
    x0f, y0f = torch.floor(x), torch.floor(y)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1)
    y0, y1 = y0.clamp(0, H - 1), y1.clamp(0, H - 1)
    flat = bev_nhwc.reshape(B, H * W, C)

    def at(yy, xx):
        return torch.gather(flat, 1, (yy * W + xx).unsqueeze(-1).expand(-1, -1, C))
    wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
    wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return at(y0, x0) * wa.unsqueeze(-1) + at(y1, x0) * wb.unsqueeze(-1) + at(y0, x1) * wc.unsqueeze(-1) + at(y1, x1) * wd.unsqueeze(-1)


def roi_grid_points(rois, grid_size):
    """rois (R, 7) -> global grid points (R, grid^3, 3) (pvrcnn_head.py:120-143)."""
    R = rois.shape[0]
    # (g^3, 3) [x, y, z] index == ones(g, g, g).nonzero() of the reference, built without its host sync (nonzero reads a count back)
    ax = torch.arange(grid_size, device=rois.device, dtype=torch.float32)
    idx = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).view(-1, 3)
    size = rois[:, 3:6].unsqueeze(1)
    local = (idx.unsqueeze(0) + 0.5) / grid_size * size - size / 2
    glob = common_utils.rotate_points_along_z(local.clone(), rois[:, 6]) + rois[:, 0:3].unsqueeze(1)
    return glob.view(R, -1, 3)


def fc_stack(cin, widths, cout, dropout=0.0):
    """RoIHeadTemplate.make_fc_layers (roi_head_template.py:30-43): Conv1d(k=1)/BN/ReLU blocks (+ dropout after the first),
    then a biased Conv1d to `cout`"""
    layers, c = [], cin
    for k, w in enumerate(widths):
        layers += [nn.Conv1d(c, w, kernel_size=1, bias=False), nn.BatchNorm1d(w), nn.ReLU()]
        c = w
        if dropout >= 0 and k == 0:
            layers.append(nn.Dropout(dropout))
    layers.append(nn.Conv1d(c, cout, kernel_size=1, bias=True))
    return nn.Sequential(*layers)


class DenseChain:
    """Eval-mode view of a Sequential of (Conv1d(k=1) | Linear) [+ BatchNorm1d] [+ ReLU] [+ Dropout] blocks as a chain of row-major
    GEMMs: BatchNorm folded into the weights, shift + ReLU in the GEMM epilogue, dropout gone.  The reference applies these
    stacks as Conv1d over (rows, C, 1) tensors (roi_head_template.py:30-43, pvrcnn_head.py:150-160): on this stack that is one
    degenerate convolution plus a BatchNorm launch tuned for images per layer (~0.2 ms each on 800 rows).  Folded operands
    are cached until a parameter changes."""

    def __init__(self, seq):
        self.seq, self.key, self.layers = seq, None, None

    def _fold(self):
        mods = list(self.seq)
        srcs = [t for m in mods for t in (getattr(m, "weight", None), getattr(m, "bias", None), getattr(m, "running_mean", None),
                                          getattr(m, "running_var", None)) if t is not None]
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        if key == self.key:
            return self.layers
        layers, i = [], 0
        with torch.no_grad():
            while i < len(mods):
                m = mods[i]
                assert isinstance(m, (nn.Conv1d, nn.Linear)), f"DenseChain: unexpected {type(m).__name__}"
                w = (m.weight[:, :, 0] if isinstance(m, nn.Conv1d) else m.weight).t()             # (Cin, Cout)
                shift = m.bias if m.bias is not None else w.new_zeros(w.shape[1])
                i += 1
                if i < len(mods) and isinstance(mods[i], nn.BatchNorm1d):
                    bn = mods[i]
                    assert not bn.training, "DenseChain folds eval-mode BatchNorm only"
                    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
                    w, shift = w * scale.view(1, -1), (shift - bn.running_mean) * scale + bn.bias
                    i += 1
                relu = i < len(mods) and isinstance(mods[i], nn.ReLU)
                i += int(relu)
                if i < len(mods) and isinstance(mods[i], nn.Dropout):
                    i += 1
                layers.append((w.contiguous(), shift.contiguous(), relu))
        self.key, self.layers = key, layers
        return layers

    def __call__(self, x):
        """x (rows, Cin) -> (rows, Cout)"""
        for w, shift, relu in self._fold():
            x = pn_common.addmm_act(shift, x, w, relu)
        return x


class PVRCNNKitti(SECONDKitti):
    def __init__(self, batch_size=8, max_voxels=16000, n_max=20000, device="cuda", num_keypoints=2048, grid_size=6):
        super().__init__(batch_size=batch_size, max_voxels=max_voxels, n_max=n_max, device=device)
        self.num_keypoints, self.grid_size = num_keypoints, grid_size
        self.roi_pre, self.roi_thresh, self.roi_post = 1024, 0.7, 100            # ROI_HEAD.NMS_CONFIG.TEST
        self.score_thresh, self.nms_thresh, self.nms_pre, self.nms_post = 0.1, 0.1, 4096, 500   # POST_PROCESSING
        # ---- VoxelSetAbstraction
        self.SA_rawpoints = pn_stack_modules.StackSAModuleMSG(radii=[0.4, 0.8], nsamples=[16, 16], mlps=[[1, 16, 16], [1, 16, 16]],
                                                              use_xyz=True, pool_method='max_pool')
        self.SA_layers, self.SA_layer_names, self.downsample = nn.ModuleList(), [], {}
        c_in = 256 + 32                                                          # bev + raw points
        for name, (ds, radii, ns, mlps, cin) in VSA_SOURCES.items():
            self.SA_layers.append(pn_stack_modules.StackSAModuleMSG(radii=list(radii), nsamples=list(ns),
                                                                    mlps=[[cin] + list(m) for m in mlps], use_xyz=True,
                                                                    pool_method='max_pool'))
            self.SA_layer_names.append(name)
            self.downsample[name] = ds
            c_in += sum(m[-1] for m in mlps)
        assert c_in == 640
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, 128, bias=False), nn.BatchNorm1d(128), nn.ReLU())
        # ---- PointHeadSimple (class-agnostic, on the features before fusion)
        self.point_cls_layers = nn.Sequential(nn.Linear(c_in, 256, bias=False), nn.BatchNorm1d(256), nn.ReLU(),
                                              nn.Linear(256, 256, bias=False), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, 1))
        # ---- PVRCNNHead
        self.roi_grid_pool_layer = pn_stack_modules.StackSAModuleMSG(radii=[0.8, 1.6], nsamples=[16, 16],
                                                                     mlps=[[128, 64, 64], [128, 64, 64]], use_xyz=True,
                                                                     pool_method='max_pool')
        pre = grid_size ** 3 * 128
        self.shared_fc_layer = nn.Sequential(nn.Conv1d(pre, 256, 1, bias=False), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3),
                                             nn.Conv1d(256, 256, 1, bias=False), nn.BatchNorm1d(256), nn.ReLU())
        self.cls_layers = fc_stack(256, [256, 256], 1, dropout=0.3)
        self.reg_layers = fc_stack(256, [256, 256], 7, dropout=0.3)
        for m in (self.shared_fc_layer, self.cls_layers, self.reg_layers):          # init_weights('xavier'), :52-70
            for l in m.modules():
                if isinstance(l, nn.Conv1d):
                    nn.init.xavier_normal_(l.weight)
                    if l.bias is not None:
                        nn.init.constant_(l.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)
        self.to(device).eval()
        self._dense = {n: DenseChain(getattr(self, n)) for n in ("vsa_point_feature_fusion", "point_cls_layers", "shared_fc_layer",
                                                                 "cls_layers", "reg_layers")}

    # ---- stages --------------------------------------------------------------------------------
    def trunk(self, points, point_offsets):
        """SECOND trunk -> (multi-scale sparse tensors, BEV map (B, 256, 200, 176) channels-last, merged dense-head output)"""
        feats, coords = self.voxelize_vfe(points, point_offsets)
        bd = self.backbone3d({"voxel_features": feats, "voxel_coords": coords, "batch_size": self.B})
        bev = bd["encoded_spconv_tensor"].dense_bev()
        (head,) = self.backbone_head(bev)
        return bd["multi_scale_3d_features"], bev, head

    def proposals(self, head, roi_pre=None, roi_thresh=None, roi_post=None):
        """proposal_layer (roi_head_template.py:45-99), all frames at once -> rois (B, post, 7) zero padded, roi_scores (raw
        logits), roi_labels (1-based), num (B,).  roi_pre / roi_thresh / roi_post: NMS_CONFIG's NMS_PRE_MAXSIZE / NMS_THRESH /
        NMS_POST_MAXSIZE, by default the TEST values this model was built with (train_loss passes the TRAIN ones)."""
        roi_pre = self.roi_pre if roi_pre is None else int(roi_pre)
        roi_thresh = self.roi_thresh if roi_thresh is None else float(roi_thresh)
        roi_post = self.roi_post if roi_post is None else int(roi_post)
        a, nc = self.num_anchor_per_loc, self.num_class
        cls = head[..., :a * nc].reshape(self.B, -1, nc)
        scores_all, labels_all = cls.max(dim=-1)                                   # raw logits: cls_preds_normalized is False
        k = min(roi_pre, scores_all.shape[1])
        if scores_all.is_cuda and anchor_post.topk_supported(scores_all.shape[1], k):
            # raw logits, no threshold: the exact device top-k with its signed key (csrc/topk.hip; ties by ascending anchor index)
            top_scores, top_idx, _ = anchor_post.topk_desc(scores_all.contiguous(), k, float("-inf"), score_max=float(np.finfo(np.float32).max))
        else:
            top_scores, top_idx = torch.topk(scores_all, k, dim=1)
        boxes = anchor_post.decode_topk(head, top_idx, self.anchors, a, box_off=a * nc, dir_off=a * (nc + 7),
                                        num_dir_bins=self.num_dir_bins, dir_offset=self.dir_offset,
                                        dir_limit_offset=self.dir_limit_offset)
        post = min(roi_post, k)
        keep, num = iou3d_nms_cuda.nms_batch(boxes, None, roi_thresh, max_keep=post)
        num = torch.clamp(num, max=post)
        valid = torch.arange(post, device=keep.device).unsqueeze(0) < num.unsqueeze(1)
        sel = torch.where(valid, keep[:, :post], torch.zeros_like(keep[:, :post])).clamp_(0, k - 1)
        rois = torch.gather(boxes, 1, sel.unsqueeze(-1).expand(-1, -1, 7)) * valid.unsqueeze(-1)
        roi_scores = torch.gather(top_scores, 1, sel) * valid
        roi_labels = (torch.gather(labels_all, 1, torch.gather(top_idx, 1, sel)) + 1) * valid
        return rois, roi_scores, roi_labels, num, (boxes, top_scores)

    def rcnn_targets(self, rois, roi_scores, roi_labels, gt_boxes, gt_boxes_enlarged=None, target_config=None, fg_keys=None,
                     draws=None, generator=None):
        """RoIHeadTemplate.assign_targets (roi_head_template.py:101-131) on what proposals() returns: rois (B, R, 7) zero padded,
        roi_scores (B, R), roi_labels (B, R) 1-based (0 on the padding: those rois match no gt and land in easy bg, as in the
        reference), gt_boxes (B, M, 8) [box | class id] -> the reference's targets_dict (rois, gt_of_rois in the roi's frame,
        gt_of_rois_src, gt_iou_of_rois, roi_scores, roi_labels, reg_valid_mask, rcnn_cls_labels) plus sampled_inds and
        frame_status.  One HIP launch, no host synchronisation; target_config overrides entries of pv_rcnn.yaml's TARGET_CONFIG;
        fg_keys / draws / generator: the random numbers (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py here)."""
        cfg = AttrDict(TARGET_CONFIG, **(target_config or {}))
        cached = self.__dict__.get("_rcnn_target_head")
        if cached is None or cached[0] != dict(cfg):
            cached = self.__dict__["_rcnn_target_head"] = (dict(cfg), RoIHeadTemplate(self.num_class, AttrDict(TARGET_CONFIG=cfg)))
        batch = {"batch_size": rois.shape[0], "rois": rois, "roi_scores": roi_scores, "roi_labels": roi_labels, "gt_boxes": gt_boxes}
        if gt_boxes_enlarged is not None:
            batch["gt_boxes_enlarged"] = gt_boxes_enlarged
        return cached[1].assign_targets(batch, fg_keys=fg_keys, draws=draws, generator=generator)

    def rcnn_loss(self, rcnn_cls, rcnn_reg, targets_dict, loss_config=None):
        """RoIHeadTemplate.get_loss (roi_head_template.py:222-233) on what rcnn_targets() returns and the head's rcnn_cls (B * P, 1)
        / rcnn_reg (B * P, 7) -> (loss, stats): loss = cls + reg + corner, a differentiable 0-dim tensor; stats the device record
        [cls, reg, corner, fg_sum, n_valid].  One HIP launch (one more in backward), no host synchronisation; loss_config
        overrides entries of pv_rcnn.yaml's LOSS_CONFIG."""
        cfg = dict(LOSS_CONFIG, **(loss_config or {}))
        cached = self.__dict__.get("_rcnn_loss_spec")
        if cached is None or cached[0] != cfg:
            cached = self.__dict__["_rcnn_loss_spec"] = (cfg, roi_loss.spec_from_cfg(dict(LOSS_CONFIG=cfg)))
        cls, reg, corner, stats = roi_loss.roi_head_loss(rcnn_cls, rcnn_reg, targets_dict, cached[1])
        return cls + reg + corner, stats

    def _point_spec(self, loss_config=None, target_config=None):
        cfg = dict(TARGET_CONFIG=dict(POINT_HEAD_CONFIG["TARGET_CONFIG"], **(target_config or {})),
                   LOSS_CONFIG=dict(POINT_HEAD_CONFIG["LOSS_CONFIG"], **(loss_config or {})))
        cached = self.__dict__.get("_point_head_spec")
        if cached is None or cached[0] != cfg:
            cached = self.__dict__["_point_head_spec"] = (cfg, point_head.spec_from_cfg(cfg, 1))
        return cached[1]

    def point_targets(self, kp, gt_boxes, target_config=None):
        """PointHeadSimple.assign_targets (point_head_simple.py:21-51) on what keypoints() returns: kp (B, K, 3), gt_boxes (B, M, 8)
        [box | class id] -> the reference's targets_dict (point_cls_labels (B * K) int64: 1 inside a gt, -1 in its 0.2 m shell only,
        else 0) plus point_box_idx.  One HIP launch, no host synchronisation; target_config overrides entries of pv_rcnn.yaml's
        POINT_HEAD.TARGET_CONFIG."""
        B, K = kp.shape[:2]
        bs = torch.arange(B, device=kp.device, dtype=kp.dtype).view(B, 1, 1).expand(B, K, 1)
        points = torch.cat([bs, kp], dim=-1).view(B * K, 4)
        return point_head.assign_point_targets(points, gt_boxes, self._point_spec(target_config=target_config))

    def point_loss(self, point_cls_preds, targets, loss_config=None):
        """PointHeadSimple.get_loss (point_head_simple.py:53-59) on what point_targets() returns and the head's point_cls_preds
        (B * K, 1) -> (loss, stats): the focal segmentation loss as a differentiable 0-dim tensor; stats the device record [cls, box,
        part, pos_num].  Two HIP launches (one more in backward), no host synchronisation; loss_config overrides entries of
        pv_rcnn.yaml's POINT_HEAD.LOSS_CONFIG."""
        cls, _box, _part, stats = point_head.point_head_loss(point_cls_preds, None, None, targets, self._point_spec(loss_config=loss_config))
        return cls, stats

    def keypoints(self, points, point_offsets, sizes):
        """get_sampled_points (voxel_set_abstraction.py:119-157) -> (B, num_keypoints, 3): FPS per frame, starting at point 0"""
        xyz = points[:, :3]
        if len(set(sizes)) == 1 and sizes[0] >= self.num_keypoints:                # equal-size frames: one launch for all of them
            xyz_b = xyz.reshape(self.B, sizes[0], 3).contiguous()
            idx = pn_batch.furthest_point_sample(xyz_b, self.num_keypoints).long()
            return torch.gather(xyz_b, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
        out, start = [], 0
        for n in sizes:
            cur = xyz[start:start + n].unsqueeze(0).contiguous()
            idx = pn_stack.furthest_point_sample(cur, self.num_keypoints).long()
            if n < self.num_keypoints:                                             # :142-144: wrap around
                empty = self.num_keypoints - n
                idx[0, -empty:] = idx[0, :empty]
            out.append(cur[0][idx[0]].unsqueeze(0))
            start += n
        return torch.cat(out, 0)

    def set_abstraction(self, points, sizes, kp, multi_scale, bev):
        """VoxelSetAbstraction.forward (:159-240) -> (point_features_before_fusion (B*K, 640), point_features (B*K, 128))"""
        before = self.set_abstraction_features(points, sizes, kp, multi_scale, bev)
        return before, self._dense["vsa_point_feature_fusion"](before)

    def set_abstraction_features(self, points, sizes, kp, multi_scale, bev):
        """VoxelSetAbstraction.forward up to the concatenation (:159-232) -> point_features_before_fusion (B*K, 640); in grad mode
        differentiable with respect to the BEV map, the multi-scale features and the SA layers' parameters"""
        B, K = kp.shape[0], kp.shape[1]
        dev = kp.device
        feats = []
        stride = 8
        x_idx = (kp[:, :, 0] - self.pc_range[0]) / self.voxel_size[0] / stride
        y_idx = (kp[:, :, 1] - self.pc_range[1]) / self.voxel_size[1] / stride
        feats.append(bilinear_bev(bev.permute(0, 2, 3, 1), x_idx, y_idx))          # channels-last storage: (B, H, W, C) is a view
        new_xyz = kp.reshape(-1, 3).contiguous()
        new_cnt = torch.full((B,), K, dtype=torch.int32, device=dev)
        xyz_cnt = torch.tensor(sizes, dtype=torch.int32, device=dev)
        _, f = self.SA_rawpoints(xyz=points[:, :3].contiguous(), xyz_batch_cnt=xyz_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt,
                                 features=points[:, 3:].contiguous())
        feats.append(f.view(B, K, -1))
        for layer, name in zip(self.SA_layers, self.SA_layer_names):
            t = multi_scale[name]
            xyz = common_utils.get_voxel_centers(t.indices[:, 1:4], self.downsample[name], self.voxel_size, self.pc_range)
            # rows per frame (rows are grouped by frame, frames ascending) — a comparison table instead of bincount, which
            # reads its output size back to the host
            cnt = (t.indices[:, 0:1] == torch.arange(B, device=dev, dtype=t.indices.dtype).view(1, B)).sum(0).int()
            _, f = layer(xyz=xyz.contiguous(), xyz_batch_cnt=cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt,
                         features=t.features.contiguous())
            feats.append(f.view(B, K, -1))
        return torch.cat(feats, dim=2).view(B * K, -1)

    def roi_grid_pool(self, rois, kp, point_features, point_scores):
        """roi_grid_pool (pvrcnn_head.py:73-118) -> (B*R, 128 * 216) pooled features, channel-major per RoI as the shared FC reads
        them; in grad mode differentiable with respect to point_features and point_scores"""
        B, R = rois.shape[0], rois.shape[1]
        dev = rois.device
        weighted = point_features * point_scores.view(-1, 1)                        # :88
        grid = roi_grid_points(rois.reshape(-1, 7), self.grid_size).view(B, -1, 3)  # (B, R * 216, 3)
        new_xyz = grid.reshape(-1, 3).contiguous()
        new_cnt = torch.full((B,), grid.shape[1], dtype=torch.int32, device=dev)
        xyz_cnt = torch.full((B,), kp.shape[1], dtype=torch.int32, device=dev)
        _, pooled = self.roi_grid_pool_layer(xyz=kp.reshape(-1, 3).contiguous(), xyz_batch_cnt=xyz_cnt, new_xyz=new_xyz,
                                             new_xyz_batch_cnt=new_cnt, features=weighted.contiguous())
        g3 = self.grid_size ** 3
        return pooled.view(B * R, g3, -1).permute(0, 2, 1).contiguous().view(B * R, -1)          # (B*R, C * 216): :150-153

    def roi_head(self, rois, kp, point_features, point_scores):
        """PVRCNNHead.forward, test mode (:145-177) -> rcnn_cls (B*R, 1), decoded boxes (B, R, 7)"""
        B, R = rois.shape[0], rois.shape[1]
        pooled = self.roi_grid_pool(rois, kp, point_features, point_scores)
        shared = self._dense["shared_fc_layer"](pooled)
        rcnn_cls = self._dense["cls_layers"](shared)                                             # (B*R, 1)
        rcnn_reg = self._dense["reg_layers"](shared)                                             # (B*R, 7)
        # generate_predicted_boxes (roi_head_template.py:235-263): ResidualCoder against the RoI moved to the origin
        local = rois.clone()
        local[:, :, 0:3] = 0
        dec = self.decode_residual(rcnn_reg.view(B, R, 7), local).view(-1, 7)
        dec = common_utils.rotate_points_along_z(dec.unsqueeze(1), rois[:, :, 6].reshape(-1)).squeeze(1)
        dec[:, 0:3] += rois[:, :, 0:3].reshape(-1, 3)
        return rcnn_cls, dec.view(B, R, 7)

    @staticmethod
    def decode_residual(enc, anchors):
        """ResidualCoder.decode_torch (box_coder_utils.py:45-77), 7 values"""
        xa, ya, za, dxa, dya, dza, ra = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, dxt, dyt, dzt, rt = torch.split(enc, 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        return torch.cat([xt * diagonal + xa, yt * diagonal + ya, zt * dza + za, torch.exp(dxt) * dxa, torch.exp(dyt) * dya,
                          torch.exp(dzt) * dza, rt + ra], dim=-1)

    def final_nms(self, rcnn_cls, boxes, roi_labels):
        """post_processing, class-agnostic branch with roi_labels (detector3d_template.py:236-262), all frames at once"""
        B, R = boxes.shape[0], boxes.shape[1]
        scores = torch.sigmoid(rcnn_cls.view(B, R))
        masked = torch.where(scores >= self.score_thresh, scores, scores.new_full((), -1.0))
        k = min(self.nms_pre, R)
        if masked.is_cuda and R >= 4096 and anchor_post.topk_supported(R, k, self.score_thresh):     # (100 RoIs per frame: torch.topk)
            top, idx, counts = anchor_post.topk_desc(masked.contiguous(), k, self.score_thresh)
        else:
            top, idx = torch.topk(masked, k, dim=1)
            counts = (top >= self.score_thresh).sum(1).to(torch.int32)
        cand = torch.gather(boxes, 1, idx.unsqueeze(-1).expand(-1, -1, 7)).contiguous()
        post = min(self.nms_post, k)
        keep, num = iou3d_nms_cuda.nms_batch(cand, counts, self.nms_thresh, max_keep=post)
        num = torch.clamp(num, max=post)
        valid = torch.arange(post, device=keep.device).unsqueeze(0) < num.unsqueeze(1)
        sel = torch.where(valid, keep[:, :post], torch.zeros_like(keep[:, :post])).clamp_(0, k - 1)
        return (torch.gather(cand, 1, sel.unsqueeze(-1).expand(-1, -1, 7)), torch.gather(top, 1, sel),
                torch.gather(roi_labels, 1, torch.gather(idx, 1, sel)), num)

    # ---- training ------------------------------------------------------------------------------
    def train_loss(self, points, point_offsets, sizes, gt_boxes, host_offsets=None, backbone="stock", sparse="stock",
                   wgrad="library", deblock="library", sa="stock", target_config=None, fg_keys=None, draws=None, generator=None):
        """One training forward of PV-RCNN-KITTI (pv_rcnn.py get_training_loss and the modules it calls) on this package's kernels
        -> (rpn_cls, rpn_loc, rpn_dir, point_loss, rcnn_loss), differentiable with respect to every parameter; the step's loss is
        their sum.  points / point_offsets / sizes as forward(); gt_boxes (B, M, 8) [box | class id].
          1. SECOND's grad-mode trunk (SECONDKitti.train_trunk: backbone / sparse / wgrad / deblock as there) and rpn_loss;
          2. proposals() without gradient at NMS_CONFIG.TRAIN (pre 9000, post 512, threshold 0.8), rcnn_targets (target_config,
             fg_keys, draws, generator as there) and the keypoints (no gradient);
          3. the set abstraction in grad mode and the fusion / point-head modules (train-mode BatchNorm1d); point_targets /
             point_loss on the features before fusion; point_scores = sigmoid(point_cls_preds).max(-1), NOT detached
             (point_head_simple.py:83-84, pvrcnn_head.py:91);
          4. RoI-grid pooling on the sampled rois, shared_fc_layer / cls_layers / reg_layers as modules (Dropout live), rcnn_loss.
        sa: "stock" (the StackSAModuleMSG modules as torch runs them: (M, C, nsample) groups, Conv2d / BatchNorm2d / ReLU, and the
        grouping gradient's float atomicAdd) or "fused" (sa_train.fused_sa_train: DESIGN §3.31).
        Host synchronisations: those of the trunk.  Not bitwise reproducible as a whole (library GEMMs, the index_put gradient of
        bilinear_bev): DESIGN §3.31."""
        from . import sa_train
        err = roi_loss._lib.LidarHipError
        if not self.training:
            raise err("PVRCNNKitti.train_loss needs train mode (call .train() first)")
        if sa not in ("stock", "fused"):
            raise err(f"PVRCNNKitti.train_loss: sa must be 'stock' or 'fused', got {sa!r}")
        head, multi_scale, bev = self.train_trunk(points, point_offsets, host_offsets, backbone, sparse, wgrad, deblock,
                                                  "PVRCNNKitti.train_loss")
        rpn_cls, rpn_loc, rpn_dir = self.rpn_loss(head, gt_boxes)
        with torch.no_grad():
            # the three head outputs in the merged layout proposals() reads: (B, locations, [cls | box | dir] of the location's anchors)
            merged = torch.cat([t.reshape(self.B, -1, t.shape[-1] * self.num_anchor_per_loc) for t in head], dim=-1).contiguous()
            rois, roi_scores, roi_labels, _, _ = self.proposals(merged, roi_pre=9000, roi_thresh=0.8, roi_post=512)
            targets = self.rcnn_targets(rois, roi_scores, roi_labels, gt_boxes, target_config=target_config, fg_keys=fg_keys,
                                        draws=draws, generator=generator)
            kp = self.keypoints(points, point_offsets, sizes)
        with sa_train.fused_sa_train(sa == "fused"):
            before = self.set_abstraction_features(points, sizes, kp, multi_scale, bev)
            fused = self.vsa_point_feature_fusion(before)
            point_cls_preds = self.point_cls_layers(before)                          # (B * K, 1)
            point_loss, _ = self.point_loss(point_cls_preds, self.point_targets(kp, gt_boxes))
            point_scores = torch.sigmoid(point_cls_preds).max(dim=-1)[0]
            pooled = self.roi_grid_pool(targets["rois"], kp, fused, point_scores)
        shared = self.shared_fc_layer(pooled.unsqueeze(-1))                          # Conv1d stacks over (rows, C, 1): :150-160
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_loss, _ = self.rcnn_loss(rcnn_cls, rcnn_reg, targets)
        return rpn_cls, rpn_loc, rpn_dir, point_loss, rcnn_loss

    def train_step(self, points, point_offsets, sizes, gt_boxes, optimizer, **train_loss_kwargs):
        """One training iteration as PointPillarKITTI.train_step runs it, with optimizer = optim.AdamOneCycle(self, ...): zero_grad,
        train_loss, backward of the sum of its five terms, optimizer.step().  -> (rpn_cls, rpn_loc, rpn_dir, point_loss, rcnn_loss,
        total_norm), detached device tensors; total_norm is the gradient norm before clipping."""
        optimizer.zero_grad()
        losses = self.train_loss(points, point_offsets, sizes, gt_boxes, **train_loss_kwargs)
        sum(losses).backward()
        total_norm = optimizer.step()
        return (*[t.detach() for t in losses], total_norm)

    @torch.no_grad()
    def forward(self, points, point_offsets, sizes):
        """points (sum N, 4), point_offsets (B+1) i32 device, sizes = the same frame sizes as a host list"""
        # furthest-point sampling needs the raw points only and occupies one CU per frame for ~2 ms: it runs on a side stream
        # under the trunk (sparse + BEV backbone, which fill the other CUs) instead of after it
        dev = points.device
        cur = torch.cuda.current_stream(dev)
        side = self.__dict__.get("_kp_stream")
        if side is None:
            side = self.__dict__["_kp_stream"] = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            kp = self.keypoints(points, point_offsets, sizes)
        multi_scale, bev, head = self.trunk(points, point_offsets)
        rois, roi_scores, roi_labels, _, _ = self.proposals(head)
        cur.wait_stream(side)
        kp.record_stream(cur)
        before, fused = self.set_abstraction(points, sizes, kp, multi_scale, bev)
        point_scores = torch.sigmoid(self._dense["point_cls_layers"](before)).max(dim=-1)[0]
        rcnn_cls, boxes = self.roi_head(rois, kp, fused, point_scores)
        return self.final_nms(rcnn_cls, boxes, roi_labels)
