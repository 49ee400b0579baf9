"""ATSSTargetAssigner with the reference's name and assign_targets contract
(pcdet/models/dense_heads/target_assigner/atss_target_assigner.py; ATSS, https://arxiv.org/abs/1912.02424), run as one batched
HIP call (lidardetection_amd/atss_assign.py, csrc/atss_assign.hip): no per-frame / per-set Python loop, no IoU or distance
matrix, no host round trip.

What the reference leaves to torch's kernels is fixed here: top-k by ascending (distance, anchor index); an anchor positive for
several gts takes the largest IoU, then the lowest gt; a gt's argmax over a set is the lowest anchor index; of several gts
forcing one anchor the highest gt index wins.  Labels are int32 (the reference's are float, as the class column is) and weights
float32, as in the AxisAlignedTargetAssigner mirror.  The centre-in-box test keeps the reference's column swap (local x against
dy / 2, local y against dx / 2, :109-110).

Two deliberate differences in the call forms.  The reference's own anchor head builds this class with a `use_multihead=`
keyword and calls assign_targets(..., gt_boxes_enlarged=...) (anchor_head_template.py:57-62, :97-99); the reference class
accepts neither, so that path raises TypeError there.  This class accepts both so the configuration works: the constructor's
use_multihead is the default of the call (an explicit use_multihead in the call overrides it), and gt_boxes_enlarged must be
None (ATSS never encodes enlarged boxes; anything else raises NotImplementedError).

`box_coder` is duck-typed: `code_size` and `encode_angle_by_sincos` (ResidualCoder) are all that is read.
"""
import torch

from ..... import atss_assign


class ATSSTargetAssigner(object):
    def __init__(self, topk, box_coder, match_height=False, use_multihead=False):
        self.topk = int(topk)
        self.box_coder = box_coder
        self.match_height = bool(match_height)
        self.use_multihead = bool(use_multihead)
        if not atss_assign.MIN_TOPK <= self.topk <= atss_assign.MAX_TOPK:
            raise ValueError(f"ATSSTargetAssigner: TOPK must be {atss_assign.MIN_TOPK}..{atss_assign.MAX_TOPK}, got {topk} "
                             "(TOPK 1 makes the reference's std NaN)")
        self._anchor_cache = (None, None)

    def _prepared_anchors(self, anchors_list, use_multihead):
        """the per-set anchors flattened in output order ((n_k, D) contiguous), cached while the anchor tensors are unchanged
        (the reference permutes the multihead anchors on every call)"""
        key = (use_multihead,) + tuple((a.data_ptr(), a._version, tuple(a.shape), str(a.device)) for a in anchors_list)
        if self._anchor_cache[0] == key:
            return self._anchor_cache[1][0]
        flat = []
        for a in anchors_list:
            if use_multihead:
                a = a.permute(3, 4, 0, 1, 2, 5)
            flat.append(a.contiguous().view(-1, a.shape[-1]))
        self._anchor_cache = (key, (flat, list(anchors_list)))   # the originals are held so their storage is not reused while cached
        return flat

    def assign_targets(self, anchors_list, gt_boxes_with_classes, use_multihead=None, gt_boxes_enlarged=None):
        """
        Args:
            anchors_list: [(z, y, x, num_size, num_rot, D), ...] or one such tensor (use_multihead needs the 6-d form)
            gt_boxes_with_classes: (B, M, C + 1) boxes and class id
            use_multihead: None (the constructor's) or bool
            gt_boxes_enlarged: must be None
        Returns:
            box_cls_labels (B, N) int32, box_reg_targets (B, N, code_size) float32, reg_weights (B, N) float32; the sets are
            concatenated along dim 1, on the single-head path too (the reference does not interleave them per location)
        """
        if gt_boxes_enlarged is not None:
            raise NotImplementedError("ATSSTargetAssigner: gt_boxes_enlarged is not used by ATSS (the reference class does not "
                                      "take the argument at all)")
        if not isinstance(anchors_list, (list, tuple)):
            anchors_list = [anchors_list]
        multihead = self.use_multihead if use_multihead is None else bool(use_multihead)
        flat = self._prepared_anchors(list(anchors_list), multihead)
        labels, targets, weights = atss_assign.assign(
            flat, gt_boxes_with_classes.contiguous(), self.topk, self.box_coder.code_size,
            sincos=getattr(self.box_coder, 'encode_angle_by_sincos', False), match_height=self.match_height)
        return {
            'box_cls_labels': labels,
            'box_reg_targets': targets,
            'reg_weights': weights,
        }
