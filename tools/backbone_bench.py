"""Dense 2D backbone + head of PointPillar-KITTI (bs 16, fp32): stock modules vs the folded-BN fast path
(lidardetection_amd/bev_backbone.py), plus a probe of torch's fused MIOpen conv+bias+relu op."""
import os, sys
import torch, torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd.pointpillar import PointPillarKITTI
from _measure import host_ms
dev = torch.device("cuda:0")
m = PointPillarKITTI(batch_size=16, device=dev).randomize_for_bench(0)
x = torch.randn(16, 64, 496, 432, device=dev)
x[:, :, ::3] = 0
x = x.contiguous(memory_format=torch.channels_last)


def run(fn, n=10):
    with torch.no_grad():
        return host_ms(fn, n, warmup=3)


print("stock modules (channels_last)  %.2f ms" % run(lambda: m.backbone_head_stock(x)), flush=True)
print("folded + HIP epilogue          %.2f ms" % run(lambda: m.backbone_head(x)), flush=True)
bev = m._bev
print("  features only                %.2f ms" % run(lambda: bev.features(x)), flush=True)
with torch.no_grad():
    a, b = m.split_heads(m.backbone_head(x)[0]), m.backbone_head_stock(x)
print("max abs diff cls %.2e box %.2e dir %.2e" % tuple((p - q).abs().max().item() for p, q in zip(a, b)))
# probe: MIOpen fusion plan conv+bias+relu through torch
try:
    c0, c1 = bev.stages[0][0][:2]
    w, bb, stride, pad = c1.weight, c1.shift, c1.stride, c1.pad
    y0 = F.conv2d(x, c0.weight, None, 2, 1)
    from lidardetection_amd.bev_backbone import bias_act_
    bias_act_(y0, c0.shift)
    ref = torch.relu(F.conv2d(y0, w, bb, stride, pad))
    got = torch.miopen_convolution_relu(y0, w, bb, list(stride), list(pad), [1, 1], 1)
    print("miopen_convolution_relu diff %.2e" % (got - ref).abs().max().item())
    print("  conv + HIP epilogue  %.3f ms" % run(lambda: bias_act_(F.conv2d(y0, w, None, stride, pad), bb), 20))
    print("  miopen conv_relu     %.3f ms" % run(lambda: torch.miopen_convolution_relu(y0, w, bb, list(stride), list(pad), [1, 1], 1), 20))
    print("  conv only            %.3f ms" % run(lambda: F.conv2d(y0, w, None, stride, pad), 20))
except Exception as e:  # noqa: BLE001
    print("miopen_convolution_relu probe failed:", repr(e)[:300])
