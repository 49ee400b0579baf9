"""Generates tests/golden/deblock_train_ref.npz from the REFERENCE ITSELF: its own BaseBEVBackbone
(pcdet/models/backbones_2d/base_bev_backbone.py), loaded standalone from its file as make_bev_train_golden.py loads it, run on the CPU
in TRAIN mode in float64 under autograd, one step.

Configuration (the three deblock strides of bev_train's deblock="gemm" option, small enough for a committed fixture): input 16
channels, LAYER_NUMS [0, 0, 0], LAYER_STRIDES [1, 2, 2], NUM_FILTERS [16, 24, 24], UPSAMPLE_STRIDES [1, 2, 4], NUM_UPSAMPLE_FILTERS
[128, 128, 128]:
  * each block is its opening ZeroPad2d + 3x3 convolution + BatchNorm + ReLU alone (strides 1, 2, 2: maps 8 x 4, 4 x 2, 2 x 1);
  * deblocks: ConvTranspose2d 16 -> 128 (s = 1), 24 -> 128 (s = 2), 24 -> 128 (s = 4): all three take the gradient kernels of
    csrc/deconv_train.hip, the s = 2 and s = 4 ones the forward kernel of csrc/deconv_gemm.hip too (s = 1: s^2 C_up % 512 != 0);
    their BatchNorms are one fused call into the 384-channel concatenated map.
Input 2 x 16 x 8 x 4.  Conv / deconv weights, the input and the upstream gradient G are int8 codes times a power of two (so the
float32 values a test rebuilds are exactly what the reference ran with); the loss is sum(spatial_features_2d * G).  BatchNorm
parameters and running statistics are float32, a quarter of the gammas negative.
Stored (the same kinds of arrays as bev_train_ref.npz): inputs (`x_code`, `g_code` and their scales, `bev.<state_dict key>`: int8
weight codes with `weight_scale`, float32 BN entries), the output `out64` (float32-rounded), the input gradient `dx64`, every BN's
`d_gamma` / `d_beta` and its running statistics after the step (`rm1.<bn>`, `rv1.<bn>`), and every conv / deconv weight gradient as
float16 with a per-tensor power-of-two scale (`dw16.<key>`, `dw_scale.<key>`: value = dw16 * dw_scale).

Usage:  python tests/golden/make_deblock_train_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_assign_golden as mag  # noqa: E402
from make_golden import _load_file, _savez_reproducible  # noqa: E402

REF_FILE = os.path.join(mag.REF, "pcdet", "models", "backbones_2d", "base_bev_backbone.py")
CFG = dict(LAYER_NUMS=[0, 0, 0], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=[16, 24, 24], UPSAMPLE_STRIDES=[1, 2, 4],
           NUM_UPSAMPLE_FILTERS=[128, 128, 128])
CIN, B, H, W = 16, 2, 8, 4
W_SCALE, X_SCALE, G_SCALE = 2.0 ** -9, 2.0 ** -5, 2.0 ** -6


def config():
    cfg = types.SimpleNamespace(**CFG)
    cfg.get = lambda k, d=None: getattr(cfg, k, d)
    return cfg


def main():
    bev = _load_file("_ref_base_bev_backbone", REF_FILE)
    torch.manual_seed(51)
    m = bev.BaseBEVBackbone(config(), input_channels=CIN)
    g = torch.Generator().manual_seed(52)
    codes = {}
    with torch.no_grad():
        for name, mod in m.named_modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                # a ConvTranspose2d with kernel == stride sums over its input channels alone; 16 x: the codes stay inside int8
                fan_in = 16 * mod.weight.shape[0] if isinstance(mod, torch.nn.ConvTranspose2d) else mod.weight[0].numel()
                c = torch.round(torch.randn(mod.weight.shape, generator=g) * (1.0 / W_SCALE) / fan_in ** 0.5).clamp_(-127, 127)
                codes[name + ".weight"] = c.to(torch.int8)
                mod.weight.copy_(c * W_SCALE)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.running_mean.copy_(torch.empty(n).uniform_(-0.3, 0.3, generator=g))
                mod.running_var.copy_(torch.empty(n).uniform_(0.6, 1.4, generator=g))
                gamma = torch.empty(n).uniform_(0.5, 1.5, generator=g)
                gamma[torch.randperm(n, generator=g)[:n // 4]] *= -1.0            # negative gammas: the ReLU mask flips
                mod.weight.copy_(gamma)
                mod.bias.copy_(torch.empty(n).uniform_(-0.3, 0.3, generator=g))
    sd = {k: v.clone() for k, v in m.state_dict().items()}                 # float32, before the step and the cast
    x_code = torch.randint(-127, 128, (B, CIN, H, W), generator=g, dtype=torch.int32).to(torch.int8)
    out_shape = (B, sum(CFG["NUM_UPSAMPLE_FILTERS"]), H, W)
    g_code = torch.randint(-127, 128, out_shape, generator=g, dtype=torch.int32).to(torch.int8)

    m = m.double().train()
    x = (x_code.double() * X_SCALE).requires_grad_()
    y = m({"spatial_features": x})["spatial_features_2d"]
    assert tuple(y.shape) == out_shape
    (y * (g_code.double() * G_SCALE)).sum().backward()

    arrays = {"x_code": x_code.numpy(), "x_scale": np.float64(X_SCALE), "g_code": g_code.numpy(), "g_scale": np.float64(G_SCALE),
              "weight_scale": np.float32(W_SCALE), "out64": y.detach().float().numpy(), "dx64": x.grad.float().numpy()}
    for k, v in sd.items():
        arrays["bev." + k] = codes[k].numpy() if k in codes else v.numpy()
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            arrays["d_gamma." + name] = mod.weight.grad.float().numpy()
            arrays["d_beta." + name] = mod.bias.grad.float().numpy()
            arrays["rm1." + name] = mod.running_mean.float().numpy()
            arrays["rv1." + name] = mod.running_var.float().numpy()
        elif isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            dw = mod.weight.grad
            scale = 2.0 ** (int(np.ceil(np.log2(float(dw.abs().max())))) - 14)       # |dw16| < 2^14: inside the fp16 range
            arrays["dw16." + name + ".weight"] = (dw / scale).to(torch.float16).numpy()
            arrays["dw_scale." + name + ".weight"] = np.float64(scale)
    path = os.path.join(HERE, "deblock_train_ref.npz")
    _savez_reproducible(path, **arrays)
    print("deblock_train_ref.npz", out_shape, "|y|max %.3f" % float(y.detach().abs().max()), "y > 0: %.2f" % float((y > 0).double().mean()),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
