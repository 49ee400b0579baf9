"""Mirror of pcdet/models/dense_heads/point_intra_part_head.py: PointIntraPartOffsetHead, the first stage of Part-A2 (interface of
the reference, bodies of this project)."""
import torch

from ...utils import box_coder_utils
from .point_head_template import PointHeadTemplate


class PointIntraPartOffsetHead(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(model_cfg.CLS_FC, input_channels, num_class)
        self.part_reg_layers = self.make_fc_layers(model_cfg.PART_FC, input_channels, 3)
        self.box_layers = None                                # only a config with a box coder has box layers
        tcfg = model_cfg.TARGET_CONFIG
        if tcfg.get('BOX_CODER', None) is not None:
            self.box_coder = getattr(box_coder_utils, tcfg.BOX_CODER)(**tcfg.BOX_CODER_CONFIG)
            self.box_layers = self.make_fc_layers(model_cfg.REG_FC, input_channels, self.box_coder.code_size)

    def assign_targets(self, input_dict):
        """input_dict: point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> targets_dict (point_cls_labels,
        point_part_labels, point_box_labels when the head has box layers)"""
        coords, boxes = self._stack_inputs(input_dict)
        return self.assign_stack_targets(coords, boxes, ret_box_labels=self.box_layers is not None, ret_part_labels=True,
                                         set_ignore_flag=True, use_ball_constraint=False)

    def get_loss(self, tb_dict=None):
        return self._get_loss(tb_dict, box=self.box_layers is not None, part=True)

    def forward(self, batch_dict):
        """reads point_features, writes point_cls_scores (best class probability) and point_part_offset (sigmoid of the part
        logits); in training assigns the targets; a head with box layers also writes the decoded boxes outside training or with
        predict_boxes_when_training"""
        feats = batch_dict['point_features']
        logits, part = self.cls_layers(feats), self.part_reg_layers(feats)
        ret = {'point_cls_preds': logits, 'point_part_preds': part}
        if self.box_layers is not None:
            ret['point_box_preds'] = self.box_layers(feats)
        batch_dict['point_cls_scores'] = torch.sigmoid(logits).max(dim=-1).values
        batch_dict['point_part_offset'] = torch.sigmoid(part)
        if self.training:
            targets = self.assign_targets(batch_dict)
            ret.update({k: targets.get(k) for k in ('point_cls_labels', 'point_part_labels', 'point_box_labels')})
        if self.box_layers is not None and (self.predict_boxes_when_training or not self.training):
            self._decode_into(batch_dict, logits, ret['point_box_preds'])
        self.forward_ret_dict = ret
        return batch_dict
