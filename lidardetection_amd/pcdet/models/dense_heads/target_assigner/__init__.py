"""Mirror of pcdet.models.dense_heads.target_assigner: AnchorGenerator (pure torch) and AxisAlignedTargetAssigner (HIP)."""
