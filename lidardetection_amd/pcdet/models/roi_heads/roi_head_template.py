"""The target and loss sides of RoIHeadTemplate (pcdet/models/roi_heads/roi_head_template.py): the constructor's
proposal_target_layer, assign_targets (:101-131) and build_losses / get_box_reg_layer_loss / get_box_cls_layer_loss / get_loss
(:23-27, :133-233).  The canonical transform of assign_targets — gt boxes moved into the roi's frame, heading folded
into [-pi/2, pi/2] — is computed by the ProposalTargetLayer's own launch, so assign_targets only arranges the dict.  The losses run
as one fused launch (lidardetection_amd/roi_loss.py) and get_loss builds its tb_dict from one device-to-host copy; a config the fused
path refuses (CrossEntropy, a sin/cos coder, REG_TRACKING_INFO) takes a torch formulation of the reference's math.  Layers,
proposal_layer and box decoding are not mirrored."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import roi_loss
from ...._lib import cfg_get
from .target_assigner.proposal_target_layer import ProposalTargetLayer

_CORNER_SIGNS = [(1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1)]


def _smooth_l1(n, beta):
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def _corners(box):
    """boxes_to_corners_3d (pcdet/utils/box_utils.py:27-52): (m, 7) -> (m, 8, 3)"""
    off = box[:, None, 3:6] * (box.new_tensor(_CORNER_SIGNS) / 2)[None]
    c, s = torch.cos(box[:, 6])[:, None], torch.sin(box[:, 6])[:, None]
    xy = torch.stack([off[..., 0] * c - off[..., 1] * s, off[..., 0] * s + off[..., 1] * c, off[..., 2]], dim=-1)
    return xy + box[:, None, 0:3]


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=self.model_cfg.TARGET_CONFIG)
        self.forward_ret_dict = None
        self._loss_spec = None      # built on first use: a head made for the targets alone has no LOSS_CONFIG

    def assign_targets(self, batch_dict, fg_keys=None, draws=None, generator=None):
        """-> the reference's targets_dict: the ProposalTargetLayer's dict with `gt_of_rois` in the roi's canonical frame and
        `gt_of_rois_src` the rows before the transform"""
        with torch.no_grad():
            targets_dict, canonical = self.proposal_target_layer.forward_with_canonical(batch_dict, fg_keys=fg_keys, draws=draws,
                                                                                         generator=generator)
        targets_dict['gt_of_rois_src'] = targets_dict['gt_of_rois']
        targets_dict['gt_of_rois'] = canonical
        return targets_dict

    # ---------------------------------------------------------------- losses
    def build_losses(self, losses_cfg=None):
        """-> the fused path's RoILossSpec, or None for a config it refuses (the torch formulation then runs).  The reference's
        build_losses registers a WeightedSmoothL1Loss module; here the code weights live in the spec / are read from the config."""
        cfg = self.model_cfg if losses_cfg is None else dict(LOSS_CONFIG=losses_cfg, TARGET_CONFIG=cfg_get(self.model_cfg, "TARGET_CONFIG"))
        try:
            spec = roi_loss.spec_from_cfg(cfg)
        except NotImplementedError:
            spec = None
        self._loss_spec = (spec,)
        return spec

    def _spec(self):
        if self._loss_spec is None:
            self.build_losses()
        return self._loss_spec[0]

    def _fused(self, d):
        """(cls, reg, corner, stats) of the fused launch, evaluated once per forward_ret_dict"""
        cached = d.get("_roi_loss")
        if cached is None or cached[0] is not d["rcnn_cls"] or cached[1] is not d["rcnn_reg"]:
            cached = d["_roi_loss"] = (d["rcnn_cls"], d["rcnn_reg"], roi_loss.roi_head_loss(d["rcnn_cls"], d["rcnn_reg"], d, self._spec()))
        return cached[2]

    def _code_size(self):
        tcfg = cfg_get(self.model_cfg, "TARGET_CONFIG")
        ccfg = cfg_get(tcfg, "BOX_CODER_CONFIG") or {}
        return int(cfg_get(ccfg, "code_size", 7)) + (1 if cfg_get(ccfg, "encode_angle_by_sincos", False) else 0), bool(cfg_get(ccfg, "encode_angle_by_sincos", False))

    def _torch_reg_loss(self, d):
        """get_box_reg_layer_loss (:133-200) in torch -> (reg, corner or None, fg_sum tensor); nothing is written in place and
        nothing is read back"""
        loss_cfgs = cfg_get(self.model_cfg, "LOSS_CONFIG")
        tcfg = cfg_get(self.model_cfg, "TARGET_CONFIG")
        if cfg_get(loss_cfgs, "REG_LOSS") != "smooth-l1" or cfg_get(tcfg, "BOX_CODER", "ResidualCoder") != "ResidualCoder":
            raise NotImplementedError
        code_size, sincos = self._code_size()
        box = code_size - 1 if sincos else code_size                   # width of a box: the coder reads that many columns
        lw = cfg_get(loss_cfgs, "LOSS_WEIGHTS")
        rcnn_reg = d["rcnn_reg"]
        n = rcnn_reg.shape[0]
        fg = d["reg_valid_mask"].reshape(n) > 0
        fg_sum = fg.sum()
        denom = torch.clamp(fg_sum.to(rcnn_reg.dtype), min=1.0)
        roi = d["rois"].reshape(n, -1)[:, :box]
        gt = d["gt_of_rois"].reshape(n, -1)
        da, dg = torch.clamp_min(roi[:, 3:6], 1e-5), torch.clamp_min(gt[:, 3:6], 1e-5)
        diag = torch.sqrt(da[:, 0] ** 2 + da[:, 1] ** 2)
        cols = [gt[:, 0] / diag, gt[:, 1] / diag, gt[:, 2] / da[:, 2], torch.log(dg[:, 0] / da[:, 0]), torch.log(dg[:, 1] / da[:, 1]),
                torch.log(dg[:, 2] / da[:, 2])]
        cols += [torch.cos(gt[:, 6]) - 1.0, torch.sin(gt[:, 6])] if sincos else [gt[:, 6]]        # the anchor's heading is 0
        cols += [gt[:, k] - roi[:, k] for k in range(7, box)]
        if cfg_get(tcfg, "REG_TRACKING_INFO", False):
            cols += list(gt[:, box + 1:].unbind(dim=1))
        tg = torch.stack(cols, dim=1)
        tg = torch.where(torch.isnan(tg), rcnn_reg, tg)
        diff = (rcnn_reg - tg) * rcnn_reg.new_tensor([float(w) for w in lw["code_weights"]])
        per_row = _smooth_l1(diff.abs(), 1.0 / 9.0).sum(dim=1)
        reg = torch.where(fg, per_row, torch.zeros_like(per_row)).sum() / denom * lw["rcnn_reg_weight"]
        if not cfg_get(loss_cfgs, "CORNER_LOSS_REGULARIZATION", False):
            return reg, None, fg_sum
        pr = rcnn_reg[:, :code_size]
        diag_r = torch.sqrt(roi[:, 3] ** 2 + roi[:, 4] ** 2)
        xl, yl, zl = pr[:, 0] * diag_r, pr[:, 1] * diag_r, pr[:, 2] * roi[:, 5]
        c, s = torch.cos(roi[:, 6]), torch.sin(roi[:, 6])
        heading = torch.atan2(pr[:, 7] + s, pr[:, 6] + c) if sincos else pr[:, 6] + roi[:, 6]
        pred = torch.stack([xl * c - yl * s + roi[:, 0], xl * s + yl * c + roi[:, 1], zl + roi[:, 2], torch.exp(pr[:, 3]) * roi[:, 3],
                            torch.exp(pr[:, 4]) * roi[:, 4], torch.exp(pr[:, 5]) * roi[:, 5], heading], dim=1)
        gs = d["gt_of_rois_src"].reshape(n, -1)[:, :7]
        flipped = torch.cat([gs[:, :6], gs[:, 6:7] + math.pi], dim=1)
        pc = _corners(pred)
        # non-fg rows are replaced before the norm so that no gradient reaches them
        keep = fg[:, None, None]
        da_, db_ = (torch.where(keep, pc - _corners(g), torch.ones_like(pc)) for g in (gs, flipped))
        dist = torch.min(torch.norm(da_, dim=2), torch.norm(db_, dim=2))
        per_row = _smooth_l1(dist, 1.0).mean(dim=1)
        corner = torch.where(fg, per_row, torch.zeros_like(per_row)).sum() / denom * lw["rcnn_corner_weight"]
        return reg, corner, fg_sum

    def _torch_cls_loss(self, d):
        """get_box_cls_layer_loss (:202-220) in torch -> cls"""
        loss_cfgs = cfg_get(self.model_cfg, "LOSS_CONFIG")
        rcnn_cls = d["rcnn_cls"]
        labels = d["rcnn_cls_labels"].reshape(-1)
        valid = labels >= 0
        kind = cfg_get(loss_cfgs, "CLS_LOSS")
        if kind == "BinaryCrossEntropy":
            # the stable logit form, as the fused path evaluates it (equal to binary_cross_entropy(sigmoid(x), t) for |x| < 27.6)
            each = F.binary_cross_entropy_with_logits(rcnn_cls.reshape(-1), labels.to(rcnn_cls.dtype), reduction="none")
        elif kind == "CrossEntropy":
            each = F.cross_entropy(rcnn_cls, labels.long(), reduction="none", ignore_index=-1)
        else:
            raise NotImplementedError
        each = torch.where(valid, each, torch.zeros_like(each))
        return each.sum() / torch.clamp(valid.sum().to(each.dtype), min=1.0) * cfg_get(loss_cfgs, "LOSS_WEIGHTS")["rcnn_cls_weight"]

    def _terms(self, d):
        """-> (cls, reg, corner or None, record): record = device [cls, reg, corner, fg_sum, n_valid]"""
        if self._spec() is not None:
            cls, reg, corner, stats = self._fused(d)
            return cls, reg, (corner if self._spec().corner else None), stats
        cls = self._torch_cls_loss(d)
        reg, corner, fg_sum = self._torch_reg_loss(d)
        zero = torch.zeros_like(reg)
        n_valid = (d["rcnn_cls_labels"] >= 0).sum()
        stats = torch.stack([cls.detach(), reg.detach(), zero if corner is None else corner.detach(), fg_sum.to(reg.dtype),
                             n_valid.to(reg.dtype)])
        return cls, reg, corner, stats

    @staticmethod
    def _tb(record, has_corner, keys):
        """tb_dict entries from the host copy of the record; rcnn_loss_corner only with the option on and fg rows, as the
        reference logs it"""
        cls, reg, corner, fg_sum, _ = record
        corner_on = has_corner and fg_sum > 0
        tb = {"rcnn_loss_cls": cls, "rcnn_loss_reg": reg}
        if corner_on:
            tb["rcnn_loss_corner"] = corner
        tb["rcnn_loss"] = cls + reg + (corner if corner_on else 0.0)
        return {k: tb[k] for k in keys if k in tb}

    def get_box_reg_layer_loss(self, forward_ret_dict):
        """-> (rcnn_loss_reg with the corner term added, tb_dict), as the reference returns them"""
        _, reg, corner, stats = self._terms(forward_ret_dict)
        tb = self._tb(stats.tolist(), corner is not None, ("rcnn_loss_reg", "rcnn_loss_corner"))
        return (reg if corner is None else reg + corner), tb

    def get_box_cls_layer_loss(self, forward_ret_dict):
        cls, _, _, stats = self._terms(forward_ret_dict)
        return cls, self._tb(stats.tolist(), False, ("rcnn_loss_cls",))

    def get_loss(self, tb_dict=None):
        """-> (rcnn_loss, tb_dict); the whole tb_dict comes from ONE device-to-host copy of the record"""
        tb_dict = {} if tb_dict is None else tb_dict
        cls, reg, corner, stats = self._terms(self.forward_ret_dict)
        rcnn_loss = cls + reg if corner is None else cls + reg + corner
        tb_dict.update(self._tb(stats.tolist(), corner is not None, ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner", "rcnn_loss")))
        return rcnn_loss, tb_dict
