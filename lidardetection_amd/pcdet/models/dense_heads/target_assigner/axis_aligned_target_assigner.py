"""AxisAlignedTargetAssigner with the reference's name, constructor and assign_targets contract
(pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py), run as one batched HIP call
(lidardetection_amd/anchor_assign.py, csrc/anchor_assign.hip): no per-frame / per-class Python loop, no IoU matrix, no host
round trip.  Labels and weights are bit-identical to the reference; targets too, except the log / sin / cos columns of
ResidualCoder.encode_torch, which may differ by an ulp.

Covered: the deterministic path every reference config uses (POS_FRACTION < 0, MATCH_HEIGHT False), single head and
USE_MULTIHEAD, NORM_BY_NUM_EXAMPLES, gt_boxes_enlarged.  POS_FRACTION >= 0 (random fg / bg sampling) and match_height=True
(3D IoU matching) raise NotImplementedError.

SEPERATE_MULTIHEAD is read under the reference's own (misspelled) key.  The configs that mean it spell it SEPARATE_MULTIHEAD
(cbgs_second_multihead.yaml, cbgs_pp_multihead.yaml, kitti second_multihead.yaml), so the reference does not remap their
labels, and neither does this class.

`box_coder` is duck-typed: `code_size` and `encode_angle_by_sincos` (ResidualCoder) are all that is read.
"""
import numpy as np
import torch

from ..... import anchor_assign
from ....._lib import cfg_get


class AxisAlignedTargetAssigner(object):
    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        """Public attributes as the reference's: box_coder, match_height, class_names (np.ndarray), anchor_class_names,
        pos_fraction (None when < 0), sample_size, norm_by_num_examples, matched_thresholds / unmatched_thresholds
        (class name -> threshold), use_multihead, seperate_multihead and, with the latter, gt_remapping (class name -> 1-based
        position inside its RPN head).  Unsupported options are refused here rather than on the first training step."""
        super().__init__()
        gen_cfgs = list(model_cfg.ANCHOR_GENERATOR_CONFIG)
        tgt_cfg = model_cfg.TARGET_ASSIGNER_CONFIG
        if match_height:
            raise NotImplementedError("AxisAlignedTargetAssigner: match_height=True (3D IoU matching) is not implemented; "
                                      "no reference config sets MATCH_HEIGHT")
        if tgt_cfg.POS_FRACTION >= 0:
            raise NotImplementedError("AxisAlignedTargetAssigner: POS_FRACTION >= 0 (random fg/bg sampling) is not implemented; "
                                      "every reference config uses POS_FRACTION -1")
        self.box_coder, self.match_height = box_coder, match_height
        self.class_names = np.array(class_names)
        self.anchor_class_names = [g['class_name'] for g in gen_cfgs]
        self.pos_fraction, self.sample_size = None, cfg_get(tgt_cfg, 'SAMPLE_SIZE', None)
        self.norm_by_num_examples = tgt_cfg.NORM_BY_NUM_EXAMPLES
        self.matched_thresholds = {g['class_name']: g['matched_threshold'] for g in gen_cfgs}
        self.unmatched_thresholds = {g['class_name']: g['unmatched_threshold'] for g in gen_cfgs}
        self.use_multihead = cfg_get(model_cfg, 'USE_MULTIHEAD', False)
        self.seperate_multihead = cfg_get(model_cfg, 'SEPERATE_MULTIHEAD', False)   # the reference's key, misspelling included
        if self.seperate_multihead:
            self.gt_remapping = {name: pos + 1 for head in model_cfg.RPN_HEAD_CFGS
                                 for pos, name in enumerate(head['HEAD_CLS_NAME'])}

        self.class_of_id = anchor_assign.class_table(list(self.class_names), self.anchor_class_names)
        # labels are remapped on the multihead path only (:70-77)
        remapping = self.use_multihead and self.seperate_multihead
        self.remap = [self.gt_remapping[n] if remapping else 0 for n in self.anchor_class_names]
        self._anchor_cache = (None, None)

    def _prepared_anchors(self, all_anchors):
        """the per-class anchors flattened in output order ((n_k, D) contiguous) + the output layout, cached while the anchor
        tensors are unchanged (the reference permutes the multihead anchors on every call)"""
        key = tuple((a.data_ptr(), a._version, tuple(a.shape), str(a.device)) for a in all_anchors)
        if self._anchor_cache[0] == key:
            return self._anchor_cache[1]
        if len(all_anchors) != len(self.anchor_class_names):
            raise ValueError(f"expected {len(self.anchor_class_names)} anchor tensors, got {len(all_anchors)}")
        flat = []
        for a in all_anchors:
            if self.use_multihead:
                a = a.permute(3, 4, 0, 1, 2, 5)
            flat.append(a.contiguous().view(-1, a.shape[-1]))
        layout = anchor_assign.output_layout([tuple(a.shape) for a in all_anchors], self.use_multihead)
        prepared = (flat, layout, list(all_anchors))   # the originals are held so their storage is not reused while cached
        self._anchor_cache = (key, prepared)
        return prepared

    def assign_targets(self, all_anchors, gt_boxes_with_classes, gt_boxes_enlarged=None):
        """
        Args:
            all_anchors: [(z, y, x, num_size, num_rot, D), ...] per anchor class (AnchorGenerator + zero padding to code_size)
            gt_boxes_with_classes: (B, M, C + 1) boxes and class id
            gt_boxes_enlarged: None or (B, M, C + 1)
        Returns:
            box_cls_labels (B, N) int32, box_reg_targets (B, N, code_size) float32, reg_weights (B, N) float32
        """
        flat, (per_loc, out_off, a_total), _ = self._prepared_anchors(all_anchors)
        gt = gt_boxes_with_classes.contiguous()
        enl = gt_boxes_enlarged.contiguous() if gt_boxes_enlarged is not None else None
        labels, targets, weights = anchor_assign.assign(
            flat, gt, self.class_of_id, per_loc, out_off, a_total,
            [self.matched_thresholds[n] for n in self.anchor_class_names],
            [self.unmatched_thresholds[n] for n in self.anchor_class_names], self.remap, self.box_coder.code_size,
            sincos=getattr(self.box_coder, 'encode_angle_by_sincos', False),
            norm_by_num_examples=bool(self.norm_by_num_examples), gt_boxes_enlarged=enl)
        return {
            'box_cls_labels': labels,
            'box_reg_targets': targets,
            'reg_weights': weights,
        }
