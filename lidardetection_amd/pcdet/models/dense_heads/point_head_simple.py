"""Mirror of pcdet/models/dense_heads/point_head_simple.py: PointHeadSimple, the keypoint segmentation head of PV-RCNN (interface
of the reference, bodies of this project)."""
import torch

from .point_head_template import PointHeadTemplate


class PointHeadSimple(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.cls_layers = self.make_fc_layers(model_cfg.CLS_FC, input_channels, num_class)

    def assign_targets(self, input_dict):
        """input_dict: point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> targets_dict (point_cls_labels)"""
        coords, boxes = self._stack_inputs(input_dict)
        return self.assign_stack_targets(coords, boxes, set_ignore_flag=True, use_ball_constraint=False)

    def get_loss(self, tb_dict=None):
        return self._get_loss(tb_dict, box=False, part=False)

    def forward(self, batch_dict):
        """reads point_features (or point_features_before_fusion with USE_POINT_FEATURES_BEFORE_FUSION), writes point_cls_scores;
        in training also assigns the targets from point_coords and gt_boxes"""
        before = self.model_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False)
        logits = self.cls_layers(batch_dict['point_features_before_fusion' if before else 'point_features'])
        batch_dict['point_cls_scores'] = torch.sigmoid(logits).max(dim=-1).values
        self.forward_ret_dict = {'point_cls_preds': logits}
        if self.training:
            self.forward_ret_dict['point_cls_labels'] = self.assign_targets(batch_dict)['point_cls_labels']
        return batch_dict
