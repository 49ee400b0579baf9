"""The box coder of pcdet/utils/box_coder_utils.py that the point heads use: PointResidualCoder (:144-222).  Unlike the
reference's, the constructor does not call .cuda(): the mean sizes are kept as a CPU tensor and moved to the device (and dtype) of
the boxes on use, so the coder can be built and used without a GPU."""
import numpy as np
import torch


class PointResidualCoder(object):
    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        super().__init__()
        self.code_size = code_size
        self.use_mean_size = use_mean_size
        if self.use_mean_size:
            self.mean_size = torch.from_numpy(np.array(kwargs['mean_size'])).float()
            assert self.mean_size.min() > 0

    def _anchor_sizes(self, classes, like):
        assert classes.max() <= self.mean_size.shape[0]
        return torch.split(self.mean_size.to(device=like.device, dtype=like.dtype)[classes - 1], 1, dim=-1)

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """gt_boxes (N, 7 + C) [x, y, z, dx, dy, dz, heading, ...], points (N, 3), gt_classes (N) in [1, num_classes] ->
        (N, 8 + C).  The boxes are not written (the reference clamps gt_boxes[:, 3:6] in place)."""
        xg, yg, zg, dxg, dyg, dzg, rg, *cgs = torch.split(gt_boxes, 1, dim=-1)
        dxg, dyg, dzg = (torch.clamp_min(d, 1e-5) for d in (dxg, dyg, dzg))
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza = self._anchor_sizes(gt_classes, gt_boxes)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xt, yt, zt = (xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza
            dxt, dyt, dzt = torch.log(dxg / dxa), torch.log(dyg / dya), torch.log(dzg / dza)
        else:
            xt, yt, zt = xg - xa, yg - ya, zg - za
            dxt, dyt, dzt = torch.log(dxg), torch.log(dyg), torch.log(dzg)
        return torch.cat([xt, yt, zt, dxt, dyt, dzt, torch.cos(rg), torch.sin(rg), *cgs], dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """box_encodings (N, 8 + C) [x, y, z, dx, dy, dz, cos, sin, ...], points (N, 3), pred_classes (N) in [1, num_classes]
        -> boxes (N, 7 + C)"""
        xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(box_encodings, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)
        if self.use_mean_size:
            dxa, dya, dza = self._anchor_sizes(pred_classes, box_encodings)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xg, yg, zg = xt * diagonal + xa, yt * diagonal + ya, zt * dza + za
            dxg, dyg, dzg = torch.exp(dxt) * dxa, torch.exp(dyt) * dya, torch.exp(dzt) * dza
        else:
            xg, yg, zg = xt + xa, yt + ya, zt + za
            dxg, dyg, dzg = torch.exp(dxt), torch.exp(dyt), torch.exp(dzt)
        rg = torch.atan2(sint, cost)
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cts], dim=-1)
