"""ProposalTargetLayer with the reference's name, constructor, forward(batch_dict) keys and return dict
(pcdet/models/roi_heads/target_assigner/proposal_target_layer.py), run as one batched HIP launch
(lidardetection_amd/proposal_target.py, csrc/proposal_target.hip): no per-frame / per-class Python loop, no nonzero(), no host
round trip.

The reference samples on the host (np.random.permutation, np.random.rand, torch.randint).  Here the random numbers are two device
tensors, `fg_keys` (B, R) and `draws` (B, ROI_PER_IMAGE) in [0, 1): the without-replacement fg choice takes the fg candidates
with the smallest (key, roi index); every with-replacement pick for output slot s is candidates[min(floor(draws[b, s] * n),
n - 1)].  forward() draws both with torch.rand on the rois' device (optionally from `generator`) unless they are passed in, so any
run of the reference can be replayed: a permutation p becomes key[fg_inds[p[i]]] = i, an integer draw r of n becomes (r + 0.5) / n.

Beyond the reference's dict: `sampled_inds` (B, ROI_PER_IMAGE) int32 roi indices, `frame_status` (B,) int32 — nonzero for a frame
with neither fg nor bg (NaN overlaps), where the reference raises NotImplementedError and this layer returns zeros without reading
the flag back — and `max_overlaps` / `gt_assignment` of every roi.  The same launch also computes the rows of `gt_of_rois` after
the canonical transform of RoIHeadTemplate.assign_targets; `forward_with_canonical` hands them to the template beside the dict.

REG_TRACKING_INFO (multi-frame tracking targets from `locations` / `rotations_y`) raises NotImplementedError.
"""
import torch
import torch.nn as nn

from ..... import proposal_target


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        if roi_sampler_cfg.get('REG_TRACKING_INFO', False):
            raise NotImplementedError("ProposalTargetLayer: REG_TRACKING_INFO (tracking targets) is not implemented")
        if roi_sampler_cfg.CLS_SCORE_TYPE not in proposal_target.CLS_SCORE_TYPES:
            raise NotImplementedError(f"ProposalTargetLayer: CLS_SCORE_TYPE {roi_sampler_cfg.CLS_SCORE_TYPE!r}")

    def random_inputs(self, rois, generator=None):
        """-> (fg_keys (B, R), draws (B, ROI_PER_IMAGE)) uniform in [0, 1) on the rois' device"""
        B, R = rois.shape[0], rois.shape[1]
        fg_keys = torch.rand((B, R), dtype=torch.float32, device=rois.device, generator=generator)
        draws = torch.rand((B, self.roi_sampler_cfg.ROI_PER_IMAGE), dtype=torch.float32, device=rois.device, generator=generator)
        return fg_keys, draws

    def forward(self, batch_dict, fg_keys=None, draws=None, generator=None):
        """batch_dict: rois (B, R, 7 + C), roi_scores (B, R), roi_labels (B, R), gt_boxes (B, N, 7 + C + 1), optional
        gt_boxes_enlarged -> rois (B, M, 7 + C), gt_of_rois (B, M, 7 + C + 1), gt_iou_of_rois, roi_scores, roi_labels,
        reg_valid_mask (int64), rcnn_cls_labels (B, M) (int64 for CLS_SCORE_TYPE 'cls', float32 for 'roi_iou'), and the
        additions of the module docstring"""
        return self.forward_with_canonical(batch_dict, fg_keys=fg_keys, draws=draws, generator=generator)[0]

    def forward_with_canonical(self, batch_dict, fg_keys=None, draws=None, generator=None):
        """-> (forward()'s dict, its gt_of_rois after the canonical transform (B, M, 7 + C + 1)): what assign_targets needs"""
        cfg = self.roi_sampler_cfg
        rois = batch_dict['rois']
        if fg_keys is None or draws is None:
            k, d = self.random_inputs(rois, generator)
            fg_keys, draws = (k if fg_keys is None else fg_keys), (d if draws is None else draws)
        labels = batch_dict['roi_labels']
        out = proposal_target.assign(
            rois.contiguous(), batch_dict['roi_scores'].contiguous(), labels.contiguous() if labels.dtype == torch.int64 else labels.long(),
            batch_dict['gt_boxes'].contiguous(), fg_keys.contiguous(), draws.contiguous(), roi_per_image=cfg.ROI_PER_IMAGE,
            fg_ratio=cfg.FG_RATIO, reg_fg_thresh=cfg.REG_FG_THRESH, cls_fg_thresh=cfg.CLS_FG_THRESH, cls_bg_thresh=cfg.CLS_BG_THRESH,
            cls_bg_thresh_lo=cfg.CLS_BG_THRESH_LO, hard_bg_ratio=cfg.HARD_BG_RATIO,
            by_class=cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False), cls_score_type=cfg.CLS_SCORE_TYPE,
            gt_boxes_enlarged=batch_dict.get('gt_boxes_enlarged', None))
        cls_labels = out['rcnn_cls_labels']
        return ({'rois': out['rois'], 'gt_of_rois': out['gt_of_rois_src'], 'gt_iou_of_rois': out['gt_iou_of_rois'],
                'roi_scores': out['roi_scores'], 'roi_labels': out['roi_labels'], 'reg_valid_mask': out['reg_valid_mask'],
                'rcnn_cls_labels': cls_labels.long() if cfg.CLS_SCORE_TYPE == 'cls' else cls_labels,
                'sampled_inds': out['sampled_inds'], 'frame_status': out['frame_status'], 'max_overlaps': out['max_overlaps'],
                'gt_assignment': out['gt_assignment']}, out['gt_of_rois'])
