"""BaseBEVBackbone (pcdet/models/backbones_2d/base_bev_backbone.py) with the reference's constructor, forward(data_dict) and
state_dict keys.  In train mode, on a channels-last float32 CUDA map, forward runs bev_train.TrainBEVBackbone (fused train-mode
BatchNorm + ReLU, Winograd stride-1 convolutions forward and input gradient, the deblocks' BatchNorm straight into the concatenated
map); anything else computes the reference's way with the same modules."""
import torch
import torch.nn as nn

from .... import bev_train


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        get = model_cfg.get
        layer_nums, layer_strides, num_filters = [], [], []
        if get('LAYER_NUMS', None) is not None:
            layer_nums, layer_strides, num_filters = model_cfg.LAYER_NUMS, model_cfg.LAYER_STRIDES, model_cfg.NUM_FILTERS
            assert len(layer_nums) == len(layer_strides) == len(num_filters)
        up_strides, up_filters = [], []
        if get('UPSAMPLE_STRIDES', None) is not None:
            up_strides, up_filters = model_cfg.UPSAMPLE_STRIDES, model_cfg.NUM_UPSAMPLE_FILTERS
            assert len(up_strides) == len(up_filters)

        def bn(c):
            return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)

        c_in = [input_channels, *num_filters[:-1]]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for i, n in enumerate(layer_nums):
            f = num_filters[i]
            mods = [nn.ZeroPad2d(1), nn.Conv2d(c_in[i], f, kernel_size=3, stride=layer_strides[i], padding=0, bias=False), bn(f), nn.ReLU()]
            for _ in range(n):
                mods += [nn.Conv2d(f, f, kernel_size=3, padding=1, bias=False), bn(f), nn.ReLU()]
            self.blocks.append(nn.Sequential(*mods))
            if up_strides:
                s = up_strides[i]
                if s >= 1:
                    up = nn.ConvTranspose2d(f, up_filters[i], s, stride=s, bias=False)
                else:            # a fractional upsample stride is a strided convolution
                    k = int(round(1 / s))
                    up = nn.Conv2d(f, up_filters[i], k, stride=k, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(up_filters[i]), nn.ReLU()))
        c_cat = sum(up_filters)
        if len(up_strides) > len(layer_nums):
            s = up_strides[-1]
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(c_cat, c_cat, s, stride=s, bias=False), bn(c_cat), nn.ReLU()))
        self.num_bev_features = c_cat
        self.__dict__["_train_impl"] = None

    def _fused_ok(self, x):
        return self.training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and \
            x.is_contiguous(memory_format=torch.channels_last)

    def forward(self, data_dict):
        x = data_dict['spatial_features']
        if self._fused_ok(x):
            if self.__dict__["_train_impl"] is None:
                self.__dict__["_train_impl"] = bev_train.TrainBEVBackbone(self.blocks, self.deblocks)
            data_dict['spatial_features_2d'] = self.__dict__["_train_impl"](x)
            return data_dict
        ups = []                 # (the reference's per-stride maps go to a local dict it never returns: not kept here either)
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        data_dict['spatial_features_2d'] = x
        return data_dict
