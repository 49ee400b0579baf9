"""Mirror of pcdet.models.roi_heads: the second stage's training targets — RoIHeadTemplate.assign_targets (roi_head_template.py)
on the ProposalTargetLayer of target_assigner/, one HIP launch per batch.  The heads' layers, losses and box decoding are not
mirrored."""
