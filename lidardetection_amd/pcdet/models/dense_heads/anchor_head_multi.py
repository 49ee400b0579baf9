"""AnchorHeadMulti with the reference's name, constructor and loss methods (pcdet/models/dense_heads/anchor_head_multi.py:150-370),
on the fused HIP loss of AnchorHeadTemplate (anchor_head_template.py here).  What the multi-head loss changes is carried by the
loss spec: pos_cls_weight / neg_cls_weight, the per-head class columns, SEPARATE_MULTIHEAD (the correctly spelled key, read here as
the reference's AnchorHeadMulti reads it — the assigner reads SEPERATE_MULTIHEAD), add_sin_difference only with direction
predictions.  Per-head predictions (SEPARATE_MULTIHEAD) go to the kernels as separate pointers.

`rpn_heads` holds, per RPN_HEAD_CFGS entry, an object with the reference SingleHead's num_class, num_anchors_per_location and
head_label_indices; the head convolutions and forward() are not mirrored."""
import types

import numpy as np
import torch

from ...._lib import cfg_get
from .anchor_head_template import AnchorHeadTemplate


class AnchorHeadMulti(AnchorHeadTemplate):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True):
        self.separate_multihead = bool(cfg_get(model_cfg, 'SEPARATE_MULTIHEAD', False))
        names = [n for cfg in model_cfg.RPN_HEAD_CFGS for n in cfg['HEAD_CLS_NAME']]
        self._head_nc = [len(cfg['HEAD_CLS_NAME']) if self.separate_multihead else num_class for cfg in model_cfg.RPN_HEAD_CFGS]
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.rpn_heads = []
        # anchors per location of a head: as the reference's make_multihead (:176-183), each class is looked up by its position in
        # the heads' own concatenated class list (`names`), not in class_names
        for cfg, nc in zip(model_cfg.RPN_HEAD_CFGS, self._head_nc):
            per_loc = sum(self.num_anchors_per_location[names.index(c)] for c in cfg['HEAD_CLS_NAME'])
            labels = torch.from_numpy(np.array([list(class_names).index(c) + 1 for c in cfg['HEAD_CLS_NAME']]))
            self.rpn_heads.append(types.SimpleNamespace(num_class=nc, num_anchors_per_location=per_loc,
                                                        head_label_indices=labels))

    def _head_num_classes(self):
        return self._head_nc
