"""Mirror of pcdet.models.roi_heads.target_assigner: ProposalTargetLayer (HIP)."""
