"""DynamicMultiLevelNeck — host-side mirror of gaiaseg/models/necks/dynamic_multilevel_neck.py.

Connects the single-resolution feature maps of a ViT backbone to a pyramid head: per level a 1x1
``DynamicConvModule`` (the active input width comes with the feature map), a bilinear resize by
``scales[i]`` (mmseg.ops.resize(scale_factor=..), align_corners=False) and a 3x3 ``DynamicConvModule``.
The whole neck is one autograd node on the HIP kernels.

The resize goes through ``ops.bilinear``, which takes an output SIZE.  F.interpolate with a scale factor
maps coordinates with 1 / scale_factor, which equals input / output only where ``size * scale`` is a whole
number; any other combination is refused rather than resized with other weights.
"""
import torch.nn as nn

from ...core.bricks import DynamicConv2d, DynamicConvModule
from ...core.dynamic import DynamicMixin
from ...hip import ops
from ...hip.runtime import tape_function
from ..builder import NECKS


def scaled_size(size, scale):
    """floor(size * scale) as F.interpolate computes it, or ValueError where size * scale is fractional"""
    out = size * scale
    if out != int(out) or out < 1:
        raise ValueError("scales: %d x %s is not a whole number of pixels; resizing by a scale factor is "
                         "implemented for exact output sizes only" % (size, scale))
    return int(out)


@NECKS.register_module()
class DynamicMultiLevelNeck(nn.Module, DynamicMixin):
    def __init__(self, in_channels, out_channels, scales=[0.5, 1, 2, 4], conv_cfg=None, norm_cfg=None,
                 act_cfg=None):
        super().__init__()
        assert isinstance(in_channels, list)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.scales, self.num_outs = list(scales), len(scales)
        self.lateral_convs = nn.ModuleList()
        self.convs = nn.ModuleList()
        for in_channel in in_channels:
            self.lateral_convs.append(DynamicConvModule(in_channel, out_channels, kernel_size=1,
                                                        conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg))
        for _ in range(self.num_outs):
            self.convs.append(DynamicConvModule(out_channels, out_channels, kernel_size=3, padding=1, stride=1,
                                                conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg))
        self.init_weights()

    def init_weights(self):
        """xavier_init(distribution='uniform') of every conv, zero biases"""
        for m in self.modules():
            if isinstance(m, DynamicConv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward_acts(self, tape, inputs):
        assert len(inputs) == len(self.in_channels)
        laterals = [conv.forward_act(tape, inputs[i]) for i, conv in enumerate(self.lateral_convs)]
        if len(laterals) == 1:   # one input level feeds every output level
            laterals = [laterals[0]] * self.num_outs
        outs = []
        for i in range(self.num_outs):
            x = laterals[i]
            size = (scaled_size(x.H, self.scales[i]), scaled_size(x.W, self.scales[i]))
            if size != (x.H, x.W):   # a resize to the same size is the identity
                x = ops.bilinear(tape, x, size, align_corners=False)
            outs.append(self.convs[i].forward_act(tape, x))
        return outs

    def forward(self, inputs):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_acts(tape, acts), list(inputs), needs))
