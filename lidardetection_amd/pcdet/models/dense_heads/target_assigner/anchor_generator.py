"""AnchorGenerator: the reference's class name, constructor, attributes and `generate_anchors(grid_sizes)` contract
(pcdet/models/dense_heads/target_assigner/anchor_generator.py), built by broadcasting.

For anchor set k the result is a (Z, Y, X, S, R, 7) float32 tensor — bottom heights, y cells, x cells, sizes, rotations — of
boxes (x, y, z_centre, dx, dy, dz, heading), z_centre = bottom + dz / 2.  Cell centres come from torch.arange over the anchor
range: stride range / (n - 1) from the range's edge, or range / n from half a stride in when `align_center` is set.
`device` defaults to "cuda" (where the reference puts them) and may name the CPU."""
import torch


def _cell_centres(lo, hi, cells, align_center):
    if align_center:
        step = (hi - lo) / cells
        return torch.arange(lo + step / 2, hi + 1e-5, step=step, dtype=torch.float32)
    step = (hi - lo) / (cells - 1)
    return torch.arange(lo, hi + 1e-5, step=step, dtype=torch.float32)


def _anchor_set(anchor_range, grid_size, sizes, rotations, bottoms, align_center):
    xs = _cell_centres(anchor_range[0], anchor_range[3], grid_size[0], align_center)
    ys = _cell_centres(anchor_range[1], anchor_range[4], grid_size[1], align_center)
    zs = torch.tensor(bottoms, dtype=torch.float32)
    sz = torch.tensor(sizes, dtype=torch.float32).view(-1, 3)
    rot = torch.tensor(rotations, dtype=torch.float32)
    shape = (len(zs), len(ys), len(xs), len(sz), len(rot))
    # every component as a 5-axis view, broadcast to the full grid
    x = xs.view(1, 1, -1, 1, 1)
    y = ys.view(1, -1, 1, 1, 1)
    dx, dy, dz = (sz[:, q].view(1, 1, 1, -1, 1) for q in range(3))
    z = zs.view(-1, 1, 1, 1, 1) + dz / 2
    h = rot.view(1, 1, 1, 1, -1)
    return torch.stack([c.expand(shape) for c in (x, y, z, dx, dy, dz, h)], dim=-1).contiguous()


class AnchorGenerator(object):
    def __init__(self, anchor_range, anchor_generator_config):
        super().__init__()
        cfgs = list(anchor_generator_config)
        self.anchor_generator_cfg = anchor_generator_config
        self.anchor_range = anchor_range
        self.anchor_sizes = [c['anchor_sizes'] for c in cfgs]
        self.anchor_rotations = [c['anchor_rotations'] for c in cfgs]
        self.anchor_heights = [c['anchor_bottom_heights'] for c in cfgs]
        self.align_center = [c.get('align_center', False) for c in cfgs]
        self.num_of_anchor_sets = len(cfgs)

    def generate_anchors(self, grid_sizes, device="cuda"):
        """grid_sizes: one (x cells, y cells) per anchor set -> ([(Z, Y, X, S, R, 7) per set], anchors per location per set)"""
        if len(grid_sizes) != self.num_of_anchor_sets:
            raise ValueError(f"expected {self.num_of_anchor_sets} grid sizes, got {len(grid_sizes)}")
        sets = zip(grid_sizes, self.anchor_sizes, self.anchor_rotations, self.anchor_heights, self.align_center)
        anchors = [_anchor_set(self.anchor_range, g, s, r, h, a).to(device) for g, s, r, h, a in sets]
        per_location = [len(s) * len(r) * len(h) for s, r, h in zip(self.anchor_sizes, self.anchor_rotations, self.anchor_heights)]
        return anchors, per_location
