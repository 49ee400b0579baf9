"""The target side of RoIHeadTemplate (pcdet/models/roi_heads/roi_head_template.py): the constructor's proposal_target_layer and
assign_targets (:101-131).  The canonical transform of assign_targets — gt boxes moved into the roi's frame, heading folded
into [-pi/2, pi/2] — is computed by the ProposalTargetLayer's own launch, so assign_targets only arranges the dict.  Layers,
proposal_layer, losses and box decoding are not mirrored."""
import torch
import torch.nn as nn

from .target_assigner.proposal_target_layer import ProposalTargetLayer


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=self.model_cfg.TARGET_CONFIG)
        self.forward_ret_dict = None

    def assign_targets(self, batch_dict, fg_keys=None, draws=None, generator=None):
        """-> the reference's targets_dict: the ProposalTargetLayer's dict with `gt_of_rois` in the roi's canonical frame and
        `gt_of_rois_src` the rows before the transform"""
        with torch.no_grad():
            targets_dict, canonical = self.proposal_target_layer.forward_with_canonical(batch_dict, fg_keys=fg_keys, draws=draws,
                                                                                         generator=generator)
        targets_dict['gt_of_rois_src'] = targets_dict['gt_of_rois']
        targets_dict['gt_of_rois'] = canonical
        return targets_dict
