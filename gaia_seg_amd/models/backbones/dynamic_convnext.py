"""DynamicConvNeXt backbone — host-side mirror of gaiaseg/models/backbones/dynamic_convnext.py.

Same registered name, constructor signature, attribute and state-dict names, ``manipulate_body`` and
init.  ``forward`` returns logical NCHW feature maps (stored channels-last) and runs the whole backbone
as ONE autograd node over hand-written HIP kernels: the 4x4 / 2x2 strided convs and the two pointwise
"linear" layers of a block on gs_conv2d_*, the depthwise 7x7 on gs_dwconv2d_*, LayerNorm, GELU and the
layer scale + residual on csrc/convnext_ops.hip.  Activations are NHWC throughout, so the reference's
permutes between its channels_first and channels_last halves have no counterpart here.

Not implemented: stochastic depth (``drop_path_rate > 0`` is refused; the reference default is 0).
"""
import torch
import torch.nn as nn

from ...core.bricks import (DynamicConv2d, DynamicLayerNorm, DynamicLinear, build_activation_layer,
                            build_conv_layer, build_norm_layer)
from ...core.dynamic import DynamicMixin, unzip_meta
from ...hip import ops, streams
from ...hip.runtime import tape_function
from ..builder import BACKBONES

_CL_NORM = dict(type="DynLN", eps=1e-6, data_format="channels_last")
_CF_NORM = dict(type="DynLN", eps=1e-6, data_format="channels_first")


class DynamicConvNeXtBlock(nn.Module, DynamicMixin):
    """x + gamma * pwconv2(GELU(pwconv1(LN(dwconv7x7(x))))), every layer on its leading active slice."""
    search_space = {"width"}

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6, conv_cfg=dict(type="DynConv2d"),
                 norm_cfg=_CL_NORM, act_cfg=dict(type="GELU")):
        super().__init__()
        if drop_path > 0.:
            raise NotImplementedError("drop_path > 0: stochastic depth is not implemented")
        self.dwconv = build_conv_layer(conv_cfg, dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm_name, norm = build_norm_layer(norm_cfg, dim, postfix=1)
        self.add_module(self.norm_name, norm)
        self.pwconv1 = DynamicLinear(dim, 4 * dim)
        self.act = build_activation_layer(act_cfg)
        self.pwconv2 = DynamicLinear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim)) \
            if layer_scale_init_value > 0 else None
        self.init_state(width=dim)

    @property
    def norm(self):
        return getattr(self, self.norm_name)

    def manipulate_width(self, width):
        self.width_state = width
        self.dwconv.manipulate_width(width)
        self.pwconv1.manipulate_out_channels(4 * width)
        self.pwconv2.manipulate_out_channels(width)

    def forward_act(self, tape, x):
        if getattr(self, "_deploying", False) and self.gamma is not None and self.gamma.numel() != x.C:
            self.gamma = nn.Parameter(self.gamma.data[:x.C].clone(), self.gamma.requires_grad)
        y = self.dwconv.forward_act(tape, x)
        y = self.norm.forward_act(tape, y)
        y = self.pwconv1.forward_act(tape, y)
        y = self.act.forward_act(tape, y)
        y = self.pwconv2.forward_act(tape, y)
        return ops.layer_scale_add(tape, x, y, self.gamma)

    def forward(self, x):
        return tape_function(lambda tape, acts: [self.forward_act(tape, acts[0])], [x], True)[0]


class DynamicBlock(nn.ModuleList, DynamicMixin):
    """One stage: ``depth`` blocks at their maximum width, only the first ``depth_state`` run."""
    search_space = {"depth", "width"}

    def __init__(self, dim, depth, drop_path, layer_scale_init_value=1e-6, conv_cfg=dict(type="DynConv2d"),
                 norm_cfg=_CL_NORM, act_cfg=dict(type="GELU")):
        super().__init__([DynamicConvNeXtBlock(dim=dim, drop_path=drop_path[i],
                                               layer_scale_init_value=layer_scale_init_value,
                                               conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
                          for i in range(depth)])
        self.init_state(depth=depth, width=dim)

    def manipulate_depth(self, depth):
        assert depth >= 1, "Depth must be greater than 0, skipping stage is not supported yet."
        if depth > len(self):
            raise ValueError("depth %d exceeds the %d blocks of this stage" % (depth, len(self)))
        self.depth_state = depth

    def manipulate_width(self, width):
        self.width_state = width
        for m in self:   # every block, inactive ones included, as in the reference
            m.manipulate_width(width)

    def forward_act(self, tape, x):
        if getattr(self, "_deploying", False):
            del self[self.depth_state:]
        for i in range(self.depth_state):
            x = self[i].forward_act(tape, x)
        return x

    def forward(self, x):
        return tape_function(lambda tape, acts: [self.forward_act(tape, acts[0])], [x], True)[0]

    def active_blocks(self):
        return [self[i] for i in range(self.depth_state)]


@BACKBONES.register_module()
class DynamicConvNeXt(nn.Module, DynamicMixin):
    """ConvNeXt (`A ConvNet for the 2020s`, arXiv 2201.03545) with dynamic stage widths and depths."""
    search_space = {"body"}

    def __init__(self, depths, dims, in_chans=3, drop_path_rate=0., out_indices=(0, 1, 2, 3), pretrained=None,
                 layer_scale_init_value=1e-6, conv_cfg=dict(type="DynConv2d"),
                 Channels_first_norm_cfg=_CF_NORM, Channels_last_norm_cfg=_CL_NORM,
                 act_cfg=dict(type="GELU")):
        super().__init__()
        if drop_path_rate > 0:
            raise NotImplementedError("drop_path_rate > 0: stochastic depth is not implemented "
                                      "(set drop_path_rate=0, the reference default)")
        if len(depths) != 4 or len(dims) != 4:
            raise AssertionError("DynamicConvNeXt has four stages: depths and dims need four entries")
        self.depths, self.dims, self.out_indices = list(depths), list(dims), list(out_indices)
        self.init_state(body={"depth": list(depths), "width": list(dims)})
        for i in range(4):
            self.add_module("norm%d" % i, DynamicLayerNorm(dims[i], eps=1e-6, data_format="channels_first"))
        self.stem = build_conv_layer(conv_cfg, in_chans, dims[0], kernel_size=4, stride=4, padding=0)
        self.stem_ln_name, stem_ln = build_norm_layer(Channels_first_norm_cfg, dims[0], postfix=1)
        self.add_module(self.stem_ln_name, stem_ln)
        for i in (1, 2, 3):   # downsample layers: LN, then a 2x2 stride-2 conv
            name, ln = build_norm_layer(Channels_first_norm_cfg, dims[i - 1], postfix=i + 1)
            setattr(self, "ds%d_ln_name" % i, name)
            self.add_module(name, ln)
            self.add_module("ds%d_conv" % i, build_conv_layer(conv_cfg, dims[i - 1], dims[i], kernel_size=2,
                                                               stride=2, padding=0))
        self.blocks = []
        for i, depth in enumerate(depths):
            self.blocks.append("dynamic_convnext_block_%d" % (i + 1))
            self.add_module(self.blocks[-1], self.make_dynamic_convnext_block(
                dim=dims[i], depth=depth, drop_path=[0.] * depth,
                layer_scale_init_value=layer_scale_init_value, conv_cfg=conv_cfg,
                norm_cfg=Channels_last_norm_cfg, act_cfg=act_cfg))
        self.init_weights(pretrained)

    stem_ln = property(lambda self: getattr(self, self.stem_ln_name))
    ds1_ln = property(lambda self: getattr(self, self.ds1_ln_name))
    ds2_ln = property(lambda self: getattr(self, self.ds2_ln_name))
    ds3_ln = property(lambda self: getattr(self, self.ds3_ln_name))

    def make_dynamic_convnext_block(self, **kwargs):
        return DynamicBlock(**kwargs)

    # where the modules of stage i live: everything below goes through these two and the stem / ds*
    # attributes, so a subclass with other module names (DynamicConvNeXtV2) only redirects them
    def stage(self, i):
        return getattr(self, self.blocks[i])

    def out_norm(self, i):
        return getattr(self, "norm%d" % i)

    def init_weights(self, pretrained=None):
        """Truncated normal (std 0.02) conv and linear weights with zero biases, unit LayerNorms; then
        the checkpoint, if a path is given."""
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        for m in self.modules():
            if isinstance(m, DynamicConv2d):   # DynamicLinear included
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        if isinstance(pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)

    # ---- arch manipulation ----
    def manipulate_body(self, arch_meta):
        """{'width': [w1..w4], 'depth': [d1..d4]}: one entry per stage; the stem and the downsample
        convs follow the width of the stage they feed."""
        self.body_state = arch_meta
        convs = (self.stem, self.ds1_conv, self.ds2_conv, self.ds3_conv)
        for i, (conv, meta) in enumerate(zip(convs, unzip_meta(arch_meta))):
            self.stage(i).manipulate_arch(meta)
            conv.manipulate_width(meta["width"])

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        return {"body": {"width": list(self.dims), "depth": list(self.depths)}}

    # ---- execution ----
    def forward_act(self, tape, x):
        x = self.stem.forward_act(tape, x)
        x = self.stem_ln.forward_act(tape, x)
        outs = []
        for i in range(4):
            x = self.stage(i).forward_act(tape, x)
            if i == 0:
                streams.side_checkpoint(tape)   # as DynamicResNet: later layers' gradients are ready first
            if i in self.out_indices:
                outs.append(self.out_norm(i).forward_act(tape, x))
            if i < 3:
                x = getattr(self, "ds%d_ln" % (i + 1)).forward_act(tape, x)
                x = getattr(self, "ds%d_conv" % (i + 1)).forward_act(tape, x)
        return outs

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (stem, stage 1)."""
        mods = [self.stem, self.stem_ln, self.stage(0)]
        return [p for m in mods for p in m.parameters()]

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: everything but the blocks the
        depth states skip, and the output norms of stages outside ``out_indices``."""
        mods = [self.stem, self.stem_ln, self.ds1_ln, self.ds1_conv, self.ds2_ln, self.ds2_conv, self.ds3_ln,
                self.ds3_conv]
        mods += [self.out_norm(i) for i in range(4) if i in self.out_indices]
        for i in range(4):
            mods.extend(self.stage(i).active_blocks())
        return mods
