"""CPU restatement of the DeepLabV3 / DeepLabV3+ decode heads in plain torch (float64 after
``.double()``), written from mmseg's ASPPHead / DepthwiseSeparableASPPHead and mmcv's ConvModule /
DepthwiseSeparableConvModule: what tests/test_aspp_heads*.py compare the HIP heads against.

The modules carry the state-dict keys of the product heads (``load_state_dict(strict=True)`` of a
product head's state works) and the dynamic-width rule of the bricks: a conv uses the leading
``x.size(1)`` input channels of its max-size weight (a depthwise one its leading ``x.size(1)``
filters), a BatchNorm the leading ``x.size(1)`` entries of its parameters and buffers."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class RefConv(nn.Module):
    """Conv2d (stride 1) over the leading slice of a max-size weight; ``groups == in == out`` is the
    depthwise form with weight [C, 1, k, k]."""

    def __init__(self, cin, cout, k, padding=0, dilation=1, groups=1, bias=False):
        super().__init__()
        assert groups == 1 or groups == cin == cout
        self.depthwise = groups != 1
        self.k, self.padding, self.dilation = k, padding, dilation
        self.weight = nn.Parameter(torch.zeros(cout, 1 if self.depthwise else cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    def forward(self, x):
        c = x.size(1)
        if self.depthwise:
            b = self.bias[:c] if self.bias is not None else None
            return F.conv2d(x, self.weight[:c], b, 1, self.padding, self.dilation, groups=c)
        return F.conv2d(x, self.weight[:, :c], self.bias, 1, self.padding, self.dilation)

    def macs(self, x, y):
        """multiply-adds per image of one call with input x and output y"""
        per_out = self.k * self.k * (1 if self.depthwise else x.size(1))
        return y[0].numel() * per_out


class RefBN(nn.BatchNorm2d):
    def forward(self, x):
        c = x.size(1)
        if self.training and x.numel() // c <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                             % (tuple(x.shape),))
        return F.batch_norm(x, self.running_mean[:c], self.running_var[:c], self.weight[:c],
                            self.bias[:c], self.training, self.momentum, self.eps)


class RefConvModule(nn.Module):
    """conv (no bias) -> bn -> ReLU"""

    def __init__(self, cin, cout, k, padding=0, dilation=1, groups=1):
        super().__init__()
        self.conv = RefConv(cin, cout, k, padding, dilation, groups)
        self.bn = RefBN(cout)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class RefSepConvModule(nn.Module):
    def __init__(self, cin, cout, k, padding=0, dilation=1):
        super().__init__()
        self.depthwise_conv = RefConvModule(cin, cin, k, padding, dilation, groups=cin)
        self.pointwise_conv = RefConvModule(cin, cout, 1)

    def forward(self, x):
        return self.pointwise_conv(self.depthwise_conv(x))


class RefASPPHead(nn.Module):
    """``separable=False``: DeepLabV3 (ASPPHead); True: DeepLabV3+ (DepthwiseSeparableASPPHead)."""

    def __init__(self, in_channels, channels, num_classes, dilations=(1, 6, 12, 18), in_index=-1,
                 align_corners=False, separable=False, c1_in_channels=0, c1_channels=0):
        super().__init__()
        self.in_index, self.align_corners, self.separable = in_index, align_corners, separable
        self.image_pool = nn.Sequential(nn.AdaptiveAvgPool2d(1), RefConvModule(in_channels, channels, 1))
        self.aspp_modules = nn.ModuleList()
        for d in dilations:
            if d == 1:
                self.aspp_modules.append(RefConvModule(in_channels, channels, 1))
            elif separable:
                self.aspp_modules.append(RefSepConvModule(in_channels, channels, 3, d, d))
            else:
                self.aspp_modules.append(RefConvModule(in_channels, channels, 3, d, d))
        self.bottleneck = RefConvModule((len(dilations) + 1) * channels, channels, 3, 1)
        if separable:
            self.c1_bottleneck = RefConvModule(c1_in_channels, c1_channels, 1) if c1_in_channels > 0 else None
            self.sep_bottleneck = nn.Sequential(RefSepConvModule(channels + c1_channels, channels, 3, 1),
                                                RefSepConvModule(channels, channels, 3, 1))
        self.conv_seg = RefConv(channels, num_classes, 1, bias=True)

    def resize(self, x, size):
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=self.align_corners)

    def aspp_concat(self, x):
        outs = [self.resize(self.image_pool(x), x.shape[2:])] + [m(x) for m in self.aspp_modules]
        return torch.cat(outs, dim=1)

    def forward(self, inputs):
        x = inputs[self.in_index]
        out = self.bottleneck(self.aspp_concat(x))
        if self.separable:
            if self.c1_bottleneck is not None:
                c1 = self.c1_bottleneck(inputs[0])
                out = torch.cat([self.resize(out, c1.shape[2:]), c1], dim=1)
            out = self.sep_bottleneck(out)
        return self.conv_seg(out)


def count_macs(head, inputs):
    """multiply-adds per image of one forward of a Ref head, taken by forward hooks on every conv"""
    total = [0]
    hooks = [m.register_forward_hook(lambda mod, args, out: total.__setitem__(0, total[0] + mod.macs(args[0], out)))
             for m in head.modules() if isinstance(m, RefConv)]
    head.eval()                 # (one image: the image-pool BatchNorm needs running statistics)
    try:
        with torch.no_grad():
            head(inputs)
    finally:
        for h in hooks:
            h.remove()
    return total[0]


TINY = dict(in_channels=512, channels=16, num_classes=19, dilations=(1, 2, 3, 5), in_index=3)
TINY_C1 = dict(c1_in_channels=128, c1_channels=8)


def head_cfg(separable, dropout=0.0, **over):
    """product config of the tiny head the tests use (the tiny supernet's stage widths are maxima)"""
    cfg = dict(type="DynamicDepthwiseSeparableASPPHead" if separable else "DynamicASPPHead",
               conv_cfg=dict(type="DynConv2d"), dropout_ratio=dropout,
               norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
               loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), **TINY)
    if separable:
        cfg.update(TINY_C1)
    cfg.update(over)
    return cfg


def ref_head(separable, **over):
    kw = dict(TINY, separable=separable, **(TINY_C1 if separable else {}))
    kw.update(over)
    return RefASPPHead(**kw)


def randomize_head(head, seed=0):
    """random conv weights (fan-in scaled), BN affine and running statistics, classifier bias"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            elif getattr(m, "weight", None) is not None and m.weight.dim() == 4:
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def load_into_ref(ref, prod):
    sd = {k: v.detach().cpu().clone().contiguous() for k, v in prod.state_dict().items()}
    ref.load_state_dict(sd, strict=True)
    return ref
