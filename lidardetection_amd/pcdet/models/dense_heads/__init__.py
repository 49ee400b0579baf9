"""Mirror of pcdet.models.dense_heads: only the target assigner the anchor heads train with (target_assigner/)."""
