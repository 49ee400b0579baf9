"""Mirror of pcdet.models.dense_heads: the anchor heads' training side — AnchorHeadTemplate and AnchorHeadMulti with their loss
methods on the fused HIP loss (anchor_head_template.py, anchor_head_multi.py), and the target assigner they train with
(target_assigner/) — and the point heads PointHeadSimple, PointHeadBox, PointIntraPartOffsetHead and PointHeadSimpleMultiFrame with
their targets and losses on the fused HIP kernels (point_head_template.py, point_head_simple_multiframe.py).  The anchor heads' convolutions, forward() and generate_predicted_boxes are not
mirrored."""
from .point_head_box import PointHeadBox
from .point_head_simple import PointHeadSimple
from .point_head_simple_multiframe import PointHeadSimpleMultiFrame
from .point_head_template import PointHeadTemplate
from .point_intra_part_head import PointIntraPartOffsetHead

__all__ = ['PointHeadTemplate', 'PointHeadSimple', 'PointHeadBox', 'PointIntraPartOffsetHead', 'PointHeadSimpleMultiFrame']
