"""Deblock 1 of the PointPillar BEV backbone (64 -> 128 channels, stride 1) as ONE hipBLASLt call with the bias + ReLU epilogue
writing straight into its channel slice of the concatenated NHWC map, vs. torch.mm + lidar_bias_act_upsample_nhwc."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidardetection_amd.bev_backbone import bias_act_upsample_
from _measure import event_total_ms
dev = torch.device("cuda:0")
B, H, W, K, N, CT = 16, 248, 216, 64, 128, 384
torch.manual_seed(0)
x = torch.randn(B, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
uw = torch.randn(K, N, device=dev) * 0.1
ub = torch.randn(N, device=dev)
cat_a = torch.zeros(B, CT, H, W, device=dev).contiguous(memory_format=torch.channels_last)
cat_b = torch.zeros_like(cat_a)
A = x.permute(0, 2, 3, 1).reshape(B * H * W, K)


def t(fn, n=20):
    return event_total_ms(fn, n, 3) * 1e3      # us per call


def cur():
    y = torch.mm(A, uw)
    bias_act_upsample_(y, ub, B, H, W, 1, cat_a, 0)


view = cat_b.permute(0, 2, 3, 1).reshape(B * H * W, CT)[:, 0:N]
def fused():
    torch._addmm_activation(ub, A, uw, out=view)

print(f"torch.mm + bias_act_upsample: {t(cur):.1f} us")
try:
    print(f"_addmm_activation(out=slice): {t(fused):.1f} us")
    print("equal:", torch.equal(cat_a, cat_b), "max diff", float((cat_a - cat_b).abs().max()))
except Exception as e:
    print("fused failed:", repr(e)[:300])
tmp = torch.empty(B * H * W, N, device=dev)
print(f"_addmm_activation(out=contiguous tmp): {t(lambda: torch._addmm_activation(ub, A, uw, out=tmp)):.1f} us")
print(f"torch.mm alone: {t(lambda: torch.mm(A, uw)):.1f} us")
