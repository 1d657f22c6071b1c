"""DynamicSegformerHead: SegFormer's all-MLP decode head (arXiv 2105.15203), after mmseg's SegformerHead
(same constructor, attribute and state-dict names: ``convs.{i}``, ``fusion_conv``, ``conv_seg``)."""
import torch.nn as nn

from ...core.bricks import DynamicConvModule
from ...hip import ops
from ...hip.runtime import Act
from ..builder import HEADS
from .decode_head import DynamicBaseDecodeHead


@HEADS.register_module()
class DynamicSegformerHead(DynamicBaseDecodeHead):
    """One 1x1 conv module per input level to ``channels``, every level resized (bilinear) to level 0's size
    and written straight into its slice of one concat buffer in level order, a 1x1 fusion conv module,
    dropout, ``conv_seg``.  ``in_channels`` are the supernet maxima; the active widths come with the feature
    maps."""

    def __init__(self, interpolate_mode="bilinear", **kwargs):
        if interpolate_mode != "bilinear":
            raise NotImplementedError("interpolate_mode %r: only 'bilinear' is implemented" % (interpolate_mode,))
        kwargs.pop("input_transform", None)
        in_channels = kwargs.pop("in_channels")
        channels = kwargs.pop("channels")
        super().__init__(in_channels, channels, input_transform="multiple_select", **kwargs)
        self.interpolate_mode = interpolate_mode
        self.convs = nn.ModuleList([
            DynamicConvModule(in_ch, self.channels, 1, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                              act_cfg=self.act_cfg) for in_ch in self.in_channels])
        self.fusion_conv = DynamicConvModule(len(self.in_channels) * self.channels, self.channels, 1,
                                             conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg, act_cfg=self.act_cfg)

    def forward_acts(self, tape, inputs):
        x0, ch = inputs[0], self.channels
        cat = Act.empty(x0.N, x0.H, x0.W, len(inputs) * ch, x0.t.device)
        for i, (conv, x) in enumerate(zip(self.convs, inputs)):
            dst = cat.slice(i * ch, (i + 1) * ch)
            if (x.H, x.W) == (x0.H, x0.W):   # level 0: the conv module writes its slice itself
                conv.forward_act(tape, x, out=dst)
            else:
                ops.bilinear(tape, conv.forward_act(tape, x), (x0.H, x0.W), self.align_corners, out=dst)
        return self.cls_seg_act(tape, self.fusion_conv.forward_act(tape, cat))
