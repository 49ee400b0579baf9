"""AnchorHeadTemplate under the reference's class name and constructor signature (pcdet/models/dense_heads/anchor_head_template.py),
covering its training side: the loss methods get_cls_layer_loss, get_box_reg_layer_loss and get_loss run the fused HIP loss
(lidardetection_amd/anchor_loss.py, csrc/anchor_loss.hip), evaluated once per set of forward_ret_dict tensors and shared by the three
methods.  The static add_sin_difference and get_direction_target are small torch restatements of the reference's helpers (the fused
path does not call them).

Construction makes the anchors (AnchorGenerator mirror, padded with zero columns up to the coder's code size) and the target assigner
(AxisAlignedTargetAssigner mirror, or the ATSSTargetAssigner mirror for TARGET_ASSIGNER_CONFIG.NAME 'ATSS').  `box_coder` stands in for ResidualCoder with the two attributes the assigner and the loss read,
code_size and encode_angle_by_sincos.  Head convolutions, forward() and generate_predicted_boxes are not part of this mirror.

get_loss returns (rpn_loss, tb_dict) with the reference's keys; each float in tb_dict is a host synchronisation, as it is in the
reference.  anchor_loss.anchor_head_loss is the sync-free path."""
import math
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import anchor_loss
from ...._lib import cfg_get
from .target_assigner.anchor_generator import AnchorGenerator
from .target_assigner.atss_target_assigner import ATSSTargetAssigner
from .target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner


class AnchorHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, predict_boxes_when_training):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names
        self.predict_boxes_when_training = predict_boxes_when_training
        self.use_multihead = cfg_get(model_cfg, 'USE_MULTIHEAD', False)

        assigner_cfg = model_cfg.TARGET_ASSIGNER_CONFIG
        if assigner_cfg.BOX_CODER != 'ResidualCoder':
            raise NotImplementedError(f"AnchorHeadTemplate: BOX_CODER {assigner_cfg.BOX_CODER} (ResidualCoder only)")
        coder_cfg = cfg_get(assigner_cfg, 'BOX_CODER_CONFIG', {}) or {}
        by_sincos = bool(coder_cfg.get('encode_angle_by_sincos', False))
        self.box_coder = types.SimpleNamespace(code_size=int(coder_cfg.get('code_size', 7)) + int(by_sincos),
                                               encode_angle_by_sincos=by_sincos)

        per_class, self.num_anchors_per_location = self.generate_anchors(
            model_cfg.ANCHOR_GENERATOR_CONFIG, grid_size, point_cloud_range, anchor_ndim=self.box_coder.code_size)
        self.anchors = [a.cuda() for a in per_class]
        self.target_assigner = self.get_target_assigner(assigner_cfg)
        self.forward_ret_dict = {}
        self.build_losses(model_cfg.LOSS_CONFIG)
        self._loss_cache = (None, None)      # (the forward_ret_dict tensors and their versions, their three losses)
        self._anchors_cat = (None, None)

    @staticmethod
    def generate_anchors(anchor_generator_cfg, grid_size, point_cloud_range, anchor_ndim=7):
        """per anchor class, its (Z, Y, X, S, R, anchor_ndim) anchors on the feature map of its stride, and its anchors per location"""
        maps = [[int(v) // c['feature_map_stride'] for v in np.asarray(grid_size)[:2]] for c in anchor_generator_cfg]
        sets, per_loc = AnchorGenerator(point_cloud_range, anchor_generator_cfg).generate_anchors(maps, device="cpu")
        extra = anchor_ndim - 7
        if extra > 0:
            sets = [F.pad(a, (0, extra)) for a in sets]
        return sets, per_loc

    def get_target_assigner(self, anchor_target_cfg):
        if anchor_target_cfg.NAME == 'ATSS':   # the reference's own call form (anchor_head_template.py:56-62)
            return ATSSTargetAssigner(topk=anchor_target_cfg.TOPK, box_coder=self.box_coder, use_multihead=self.use_multihead,
                                      match_height=anchor_target_cfg.MATCH_HEIGHT)
        if anchor_target_cfg.NAME != 'AxisAlignedTargetAssigner':
            raise NotImplementedError(f"AnchorHeadTemplate: target assigner {anchor_target_cfg.NAME} is not mirrored")
        return AxisAlignedTargetAssigner(self.model_cfg, self.class_names, self.box_coder,
                                         match_height=anchor_target_cfg.MATCH_HEIGHT)

    def _head_num_classes(self):
        return None   # a single head over every class column; AnchorHeadMulti returns its heads' counts

    def build_losses(self, losses_cfg):
        """one loss spec replaces the reference's three loss modules; building it refuses an unsupported REG_LOSS_TYPE, code size or
        NUM_DIR_BINS here instead of on the first training step"""
        self.loss_spec = anchor_loss.spec_from_cfg(self.model_cfg, self.num_class, self._head_num_classes())

    def assign_targets(self, gt_boxes, gt_boxes_enlarged=None):
        return self.target_assigner.assign_targets(self.anchors, gt_boxes, gt_boxes_enlarged=gt_boxes_enlarged)

    def loss_anchors(self):
        """(N, D): one frame's anchors in the order the loss sees them (get_box_reg_layer_loss :175-184), cached while unchanged"""
        key = tuple((a.data_ptr(), a._version) for a in self.anchors)
        if self._anchors_cat[0] != key:
            if self.use_multihead:   # class by class, each one [size, rot, z, y, x]
                rows = [a.permute(3, 4, 0, 1, 2, 5).reshape(-1, a.shape[-1]) for a in self.anchors]
                flat = torch.cat(rows, 0)
            else:                    # the classes side by side at every location
                flat = torch.cat(self.anchors, dim=3).reshape(-1, self.anchors[0].shape[-1])
            self._anchors_cat = (key, flat.contiguous())
        return self._anchors_cat[1]

    def _fused_losses(self):
        """(cls, loc, dir) of the tensors now in forward_ret_dict: one fused call, reused by the three loss methods while the same
        tensors (same objects, not modified in place) are there.  The cache holds the tensors themselves, so none of them can be
        freed and its identity reused by a new tensor while the entry is alive."""
        d = self.forward_ret_dict
        names = ('cls_preds', 'box_preds', 'dir_cls_preds', 'box_cls_labels', 'box_reg_targets')
        objs = [d.get(n) for n in names]
        if not self._cached(objs):
            if self.num_class == 1:
                # class agnostic: the reference overwrites the positive labels with 1 in forward_ret_dict itself (:112-114)
                d['box_cls_labels'].masked_fill_(d['box_cls_labels'] > 0, 1)
            losses = anchor_loss.anchor_head_loss(d['cls_preds'], d['box_preds'], d.get('dir_cls_preds', None), d['box_cls_labels'],
                                                  d['box_reg_targets'], self.loss_anchors(), self.loss_spec)
            self._loss_cache = (self._cache_key(objs), losses)   # keyed after the relabel: its version bump is not a change
        return self._loss_cache[1]

    @staticmethod
    def _cache_key(objs):
        flat = []
        for o in objs:
            flat.extend(o if isinstance(o, (list, tuple)) else [o])
        return tuple((t, getattr(t, '_version', None)) for t in flat)

    def _cached(self, objs):
        key, new = self._loss_cache[0], self._cache_key(objs)
        return key is not None and len(key) == len(new) and all(a is b and va == vb for (a, va), (b, vb) in zip(key, new))

    def get_cls_layer_loss(self):
        cls_loss = self._fused_losses()[0]
        return cls_loss, {'rpn_loss_cls': cls_loss.item()}

    @staticmethod
    def add_sin_difference(boxes1, boxes2, dim=6):
        """column `dim` of the pair becomes sin(a1)cos(a2) and cos(a1)sin(a2): their difference is sin(a1 - a2)"""
        if dim == -1:
            raise ValueError("add_sin_difference: the angle column must be given by its position, not -1")
        a1, a2 = boxes1[..., dim:dim + 1], boxes2[..., dim:dim + 1]
        enc1, enc2 = torch.sin(a1) * torch.cos(a2), torch.cos(a1) * torch.sin(a2)
        return (torch.cat((boxes1[..., :dim], enc1, boxes1[..., dim + 1:]), dim=-1),
                torch.cat((boxes2[..., :dim], enc2, boxes2[..., dim + 1:]), dim=-1))

    @staticmethod
    def get_direction_target(anchors, reg_targets, one_hot=True, dir_offset=0, num_bins=2):
        """the heading bin of every anchor's target (heading = target + anchor heading - dir_offset, wrapped into [0, 2 pi)),
        one-hot in the anchors' dtype or as class indices"""
        heading = reg_targets[..., 6] + anchors.reshape(reg_targets.shape[0], -1, anchors.shape[-1])[..., 6]
        shifted = heading - dir_offset
        two_pi = 2 * math.pi
        wrapped = shifted - torch.floor(shifted / two_pi) * two_pi
        bins = torch.floor(wrapped / (two_pi / num_bins)).long().clamp(0, num_bins - 1)
        return F.one_hot(bins, num_bins).to(anchors.dtype) if one_hot else bins

    def get_box_reg_layer_loss(self):
        _, loc, direction = self._fused_losses()
        tb = {'rpn_loss_loc': loc.item()}
        if self.forward_ret_dict.get('dir_cls_preds', None) is None:
            return loc, tb
        tb['rpn_loss_dir'] = direction.item()
        return loc + direction, tb

    def get_loss(self):
        cls_loss, tb = self.get_cls_layer_loss()
        box_loss, box_tb = self.get_box_reg_layer_loss()
        total = cls_loss + box_loss
        return total, {**tb, **box_tb, 'rpn_loss': total.item()}

    def forward(self, **kwargs):
        raise NotImplementedError("AnchorHeadTemplate mirror: the head convolutions and forward() are not mirrored")
