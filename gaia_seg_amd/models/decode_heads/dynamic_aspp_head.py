"""DynamicASPPHead / DynamicDepthwiseSeparableASPPHead — DeepLabV3 and DeepLabV3+ decode heads with
dynamic input widths, after mmseg's ASPPHead (mmseg/models/decode_heads/aspp_head.py) and
DepthwiseSeparableASPPHead (sep_aspp_head.py).

The reference tree has neither; they sit on the OS8 / v1c supernet the repo already ships, where
mmseg's standard Cityscapes models are exactly these two.  ``in_channels`` / ``c1_in_channels`` are
the supernet maxima: every conv that reads a backbone feature slices its weight to the input's
channel count (DynConv2d semantics), so the heads need no search space of their own.

    ASPP:   cat([resize(image_pool(x))] + [m(x) for m in aspp_modules]) -> bottleneck -> cls_seg
    V3+ :   the same up to ``bottleneck``; then cat([resize(out, c1 size), c1_bottleneck(inputs[0])])
            -> sep_bottleneck -> cls_seg

Every ``torch.cat`` is fused: each branch's last kernel writes straight into its channel slice of the
concat buffer, as psp_concat does."""
import torch.nn as nn

from ...core.bricks import DynamicConvModule, DynamicDepthwiseSeparableConvModule
from ...hip import ops
from ...hip.runtime import Act, tape_function
from ..builder import HEADS
from .decode_head import DynamicBaseDecodeHead


class DynamicASPPModule(nn.ModuleList):
    """One conv per dilation rate: 1x1 for d == 1, else 3x3 with dilation = padding = d
    (aspp_head.py ASPPModule)."""

    def __init__(self, dilations, in_channels, channels, conv_cfg, norm_cfg, act_cfg):
        super().__init__()
        self.dilations = dilations
        self.in_channels, self.channels = in_channels, channels
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        for d in dilations:
            self.append(self.make_branch(d))

    def make_branch(self, d):
        return DynamicConvModule(self.in_channels, self.channels, 1 if d == 1 else 3, dilation=d,
                                 padding=0 if d == 1 else d, conv_cfg=self.conv_cfg,
                                 norm_cfg=self.norm_cfg, act_cfg=self.act_cfg)

    def forward_acts(self, tape, x, outs):
        """outs: the destination Acts (concat slices), one per dilation."""
        return [m.forward_act(tape, x, out=o) for m, o in zip(self, outs)]


class DynamicDepthwiseSeparableASPPModule(DynamicASPPModule):
    """ASPPModule whose 3x3 branches are depthwise-separable (sep_aspp_head.py)."""

    def make_branch(self, d):
        if d == 1:
            return super().make_branch(d)
        return DynamicDepthwiseSeparableConvModule(
            self.in_channels, self.channels, 3, dilation=d, padding=d, conv_cfg=self.conv_cfg,
            norm_cfg=self.norm_cfg, act_cfg=self.act_cfg)


@HEADS.register_module()
class DynamicASPPHead(DynamicBaseDecodeHead):
    """DeepLabV3 (Chen et al., "Rethinking Atrous Convolution for Semantic Image Segmentation")."""
    aspp_module_cls = DynamicASPPModule

    def __init__(self, in_channels, channels, num_classes, dilations=(1, 6, 12, 18),
                 dropout_ratio=0.1, conv_cfg=None, norm_cfg=None, act_cfg=dict(type="ReLU"),
                 in_index=-1, input_transform=None,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                 ignore_index=255, sampler=None, align_corners=False):
        super().__init__(in_channels, channels, num_classes=num_classes,
                         dropout_ratio=dropout_ratio, conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                         act_cfg=act_cfg, in_index=in_index, input_transform=input_transform,
                         loss_decode=loss_decode, ignore_index=ignore_index, sampler=sampler,
                         align_corners=align_corners)
        assert isinstance(dilations, (list, tuple))
        if input_transform is not None:
            raise NotImplementedError("%s takes one feature map (input_transform=None)"
                                      % type(self).__name__)
        self.dilations = tuple(dilations)
        # index 0 of the Sequential is the parameter-free pool: keys stay image_pool.1.conv.weight
        self.image_pool = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            DynamicConvModule(self.in_channels, self.channels, 1, conv_cfg=self.conv_cfg,
                              norm_cfg=self.norm_cfg, act_cfg=self.act_cfg))
        self.aspp_modules = self.aspp_module_cls(self.dilations, self.in_channels, self.channels,
                                                 conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                                 act_cfg=self.act_cfg)
        self.bottleneck = DynamicConvModule(
            (len(self.dilations) + 1) * self.channels, self.channels, 3, padding=1,
            conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg, act_cfg=self.act_cfg)

    def aspp_concat(self, tape, x):
        """cat([resize(image_pool(x))] + aspp_modules(x), dim=1) without materialising the pieces."""
        ch = self.channels
        nd = len(self.dilations)
        cat = Act.empty(x.N, x.H, x.W, (nd + 1) * ch, x.t.device)
        pooled = ops.adaptive_avgpool(tape, x, [1])[0]
        y = self.image_pool[1].forward_act(tape, pooled)
        ops.bilinear(tape, y, (x.H, x.W), self.align_corners, out=cat.slice(0, ch))
        self.aspp_modules.forward_acts(tape, x, [cat.slice((i + 1) * ch, (i + 2) * ch)
                                                 for i in range(nd)])
        return cat

    def forward_acts(self, tape, x):
        out = self.bottleneck.forward_act(tape, self.aspp_concat(tape, x))
        return self.cls_seg_act(tape, out)


@HEADS.register_module()
class DynamicDepthwiseSeparableASPPHead(DynamicASPPHead):
    """DeepLabV3+ (Chen et al., "Encoder-Decoder with Atrous Separable Convolution for Semantic Image
    Segmentation"): the ASPP output is upsampled to the stride-4 feature ``inputs[0]``, concatenated
    with its 1x1 projection and refined by two depthwise-separable 3x3 convs."""
    aspp_module_cls = DynamicDepthwiseSeparableASPPModule

    def __init__(self, c1_in_channels, c1_channels, **kwargs):
        super().__init__(**kwargs)
        assert c1_in_channels >= 0
        self.c1_in_channels, self.c1_channels = c1_in_channels, c1_channels
        if c1_in_channels > 0:
            self.c1_bottleneck = DynamicConvModule(c1_in_channels, c1_channels, 1,
                                                   conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                                   act_cfg=self.act_cfg)
        else:
            self.c1_bottleneck = None
        self.sep_bottleneck = nn.Sequential(
            DynamicDepthwiseSeparableConvModule(
                self.channels + c1_channels, self.channels, 3, padding=1, conv_cfg=self.conv_cfg,
                norm_cfg=self.norm_cfg, act_cfg=self.act_cfg),
            DynamicDepthwiseSeparableConvModule(self.channels, self.channels, 3, padding=1,
                                                conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                                act_cfg=self.act_cfg))

    def c1_concat(self, tape, out, c1):
        """cat([resize(out, c1 size), c1_bottleneck(c1)], dim=1): both written into their slices."""
        ch, c1c = self.channels, self.c1_channels
        cat = Act.empty(c1.N, c1.H, c1.W, ch + c1c, c1.t.device)
        ops.bilinear(tape, out, (c1.H, c1.W), self.align_corners, out=cat.slice(0, ch))
        self.c1_bottleneck.forward_act(tape, c1, out=cat.slice(ch, ch + c1c))
        return cat

    def forward_acts(self, tape, x, c1=None):
        out = self.bottleneck.forward_act(tape, self.aspp_concat(tape, x))
        if self.c1_bottleneck is not None:
            out = self.c1_concat(tape, out, c1)
        for m in self.sep_bottleneck:
            out = m.forward_act(tape, out)
        return self.cls_seg_act(tape, out)

    def forward(self, inputs):
        # the head reads the stride-4 feature inputs[0] besides inputs[in_index]
        inputs = list(inputs)
        selected = [inputs[self.in_index % len(inputs)]]
        if self.c1_bottleneck is not None:
            selected.append(inputs[0])
        needs = any(p.requires_grad for p in self.parameters())

        def runner(tape, acts):
            return [self.forward_acts(tape, *acts)]
        return tape_function(runner, selected, needs)[0]
