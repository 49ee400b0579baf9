"""Mirror of pcdet.models.dense_heads.target_assigner: AnchorGenerator (pure torch), AxisAlignedTargetAssigner and
ATSSTargetAssigner (HIP); the modules are imported by name (anchor_generator, axis_aligned_target_assigner, atss_target_assigner)."""
from . import atss_target_assigner   # noqa: F401
