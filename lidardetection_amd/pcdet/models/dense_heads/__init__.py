"""Mirror of pcdet.models.dense_heads: the anchor heads' training side — AnchorHeadTemplate and AnchorHeadMulti with their loss
methods on the fused HIP loss (anchor_head_template.py, anchor_head_multi.py), and the target assigner they train with
(target_assigner/).  Head convolutions, forward() and generate_predicted_boxes are not mirrored."""
