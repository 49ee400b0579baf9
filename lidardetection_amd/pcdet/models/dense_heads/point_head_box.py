"""Mirror of pcdet/models/dense_heads/point_head_box.py: PointHeadBox, the first stage of PointRCNN (interface of the reference,
bodies of this project)."""
import torch

from ...utils import box_coder_utils
from .point_head_template import PointHeadTemplate


class PointHeadBox(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        tcfg = model_cfg.TARGET_CONFIG
        self.box_coder = getattr(box_coder_utils, tcfg.BOX_CODER)(**tcfg.BOX_CODER_CONFIG)
        self.cls_layers = self.make_fc_layers(model_cfg.CLS_FC, input_channels, num_class)
        self.box_layers = self.make_fc_layers(model_cfg.REG_FC, input_channels, self.box_coder.code_size)

    def assign_targets(self, input_dict):
        """input_dict: point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> targets_dict (point_cls_labels,
        point_box_labels)"""
        coords, boxes = self._stack_inputs(input_dict)
        return self.assign_stack_targets(coords, boxes, ret_box_labels=True, set_ignore_flag=True, use_ball_constraint=False)

    def get_loss(self, tb_dict=None):
        return self._get_loss(tb_dict, box=True, part=False)

    def forward(self, batch_dict):
        """reads point_features (or point_features_before_fusion), writes point_cls_scores (sigmoid of the best logit); in training
        assigns the targets; outside training, or with predict_boxes_when_training, also writes the decoded boxes"""
        before = self.model_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False)
        feats = batch_dict['point_features_before_fusion' if before else 'point_features']
        logits, codes = self.cls_layers(feats), self.box_layers(feats)
        batch_dict['point_cls_scores'] = torch.sigmoid(logits.max(dim=-1).values)
        self.forward_ret_dict = {'point_cls_preds': logits, 'point_box_preds': codes}
        if self.training:
            targets = self.assign_targets(batch_dict)
            self.forward_ret_dict.update({k: targets[k] for k in ('point_cls_labels', 'point_box_labels')})
        if self.predict_boxes_when_training or not self.training:
            self._decode_into(batch_dict, logits, codes)
        return batch_dict
