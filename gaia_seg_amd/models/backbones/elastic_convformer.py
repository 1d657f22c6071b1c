"""ElasticConvformer backbone — host-side mirror of gaiaseg/models/backbones/elastic_convformer.py.

A Conformer (arXiv 2105.03889): a ResNet-bottleneck conv branch and a transformer token stream side by
side, coupled in every block by two "FCU" units.  Same registered name, constructor keywords, attribute and
state-dict names and search space as the reference.  ``forward`` returns the conv branch's four logical NCHW
feature maps at strides 4 / 8 / 16 / 32 and runs the whole backbone as ONE autograd node over hand-written
HIP kernels: convs and linears on gs_conv2d_* / gs_conv_bn_*, attention on gs_attention_*, LayerNorm and GELU
on csrc/convnext_ops.hip, and the coupling on csrc/fcu.hip:

* conv to tokens (``squeeze_block`` and the ``x_st + x_t`` after it): the reference's 1x1 conv, AvgPool2d(s),
  LayerNorm, GELU, cls-row concat and add run as ops.avgpool_ceil, the 1x1 conv ON THE POOLED MAP (an average
  and a 1x1 conv with bias commute; s^2 times fewer MACs) and ONE kernel for the rest (ops.fcu_down);
* tokens to conv (``expand_block`` and the ``x + x_t`` in front of ``fusion_block.conv2``): the tokens
  without their cls rows (ops.vit_feature_map, so the cls rows stay out of the BatchNorm statistics), the 1x1
  conv + BN + ReLU (conv_bn_act), and ONE kernel for nearest upsample + add (ops.fcu_up_add).

The search space is ``stem`` ({'width': w}) and ``body`` ({'depth': [3], 'block': {'convblock': {'width':
[3]}, 'embed_dim': {'width': D}, 'transblock': {'MHA': {'num_heads': {'num_heads': [3]}}, 'FFN':
{'feedforward_channels': {'feedforward_channels': [3 ratios]}}}}}); stage 4 always has depth 1 and takes
stage 3's width, heads and ratio.  The constructor's ``mlp_ratio`` is a multiplier (hidden width
int(dim * mlp_ratio)); a sampled ratio is tenths of the embedding width (int(r / 10 * D)).

Carried over as they are: ``train()`` always freezes ``conv1`` / ``bn1`` (eval mode, no gradients); with
``norm_eval`` every BatchNorm stays in eval mode while training; the relative-position tables of every
attention module are parameters that exist and are never read.

Departures from the reference, on purpose:

* ``norm_eval`` is a trailing constructor keyword (default True, the value the reference hard-codes), so a
  supernet can be trained from scratch with batch statistics;
* metas are only read, never overwritten;
* the feed-forward width follows the current embedding width whichever search key is handled first (the
  reference uses the embedding width of the previous call when 'transblock' comes first): the rule of
  ElasticTransformer.

Refused, each with its key in the message: ``drop_path`` / ``attn_drop`` / ``proj_drop`` > 0 (the reference's
default drop_path=0.1 therefore too), ``relative_position=True``, a ``patch_size`` other than 16 or 32 (the
reference's dw_stride list degenerates otherwise), ``depth % 3 != 0``, ``depth <= sum(body_depth)`` (an
IndexError on trans_dpr in the reference), a ``width`` whose quarter is no multiple of 4, and an input whose
height or width is no multiple of 2 * patch_size (the reference fails on ``x + x_t``).
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _BatchNorm

from ...core.bricks import (DynamicConv2d, DynamicLinear, build_activation_layer, build_conv_layer,
                            build_norm_layer, conv_bn_act)
from ...core.dynamic import DynamicMixin, freeze
from ...hip import ops, streams
from ...hip.runtime import tape_function
from ..builder import BACKBONES
from .elastic_transformer import ElasticFFN, ElasticMHA, _leaf, _nest, _refuse_positive, ffn_width

EXPANSION = 4


def _check_width(width, what="width"):
    if width <= 0 or width % (4 * EXPANSION):
        raise ValueError("%s %s: its quarter (the bottleneck width) must be a positive multiple of 4"
                         % (what, width))
    return width


class Elastic_trans_Block(nn.Module, DynamicMixin):
    """x + attn(ln1(x)), then x + mlp(ln2(x)): ElasticTransformerEncoderLayer with the embedding width as a
    state of its own."""
    search_space = {"width", "MHA", "FFN"}

    def __init__(self, dim, num_heads, mlp_ratio=4., proj_drop=0., attn_drop=0., drop_path=0.,
                 norm_cfg=dict(type="ElaLN"), act_cfg=dict(type="GELU"), num_fcs=2, relative_position=False):
        super().__init__()
        self.embed_dim_state = dim
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, dim, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.attn = ElasticMHA(embed_dim=dim, num_heads=num_heads, proj_drop=proj_drop, attn_drop=attn_drop,
                               drop_path=drop_path, relative_position=relative_position)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, dim, postfix=2)
        self.add_module(self.norm2_name, norm2)
        self.mlp = ElasticFFN(embed_dim=dim, feedforward_channels=int(dim * mlp_ratio), num_fcs=num_fcs,
                              act_cfg=act_cfg, drop_path=drop_path, dropout=proj_drop)
        self._ratio = None   # the sampled feed-forward ratio, once one has been set

    norm1 = property(lambda self: getattr(self, self.norm1_name))
    norm2 = property(lambda self: getattr(self, self.norm2_name))

    def manipulate_width(self, arch_meta):
        self.embed_dim_state = arch_meta
        self._apply_ratio()

    def manipulate_MHA(self, arch_meta):
        self.attn.manipulate_arch(arch_meta)

    def manipulate_FFN(self, arch_meta):
        self._ratio = _leaf(arch_meta, "feedforward_channels")
        self._apply_ratio()

    def _apply_ratio(self):
        if self._ratio is not None:
            self.mlp.manipulate_arch(_nest("feedforward_channels", ffn_width(self._ratio, self.embed_dim_state)))

    def active_children(self):
        return [self.norm1, self.norm2, self.mlp.layer1, self.mlp.layer2] + self.attn.active_children()

    def forward_act(self, tape, x):
        x = self.attn.forward_act(tape, self.norm1.forward_act(tape, x), residual=x)
        return self.mlp.forward_act(tape, self.norm2.forward_act(tape, x), residual=x)


class Elastic_conv_Block(nn.Module, DynamicMixin):
    """The ResNet bottleneck (expansion 4, stride on the 3x3) of the conv branch; ``x_t``, where given, is
    added to the 3x3 conv's input after a nearest upsample."""
    search_space = {"width"}

    def __init__(self, inplanes, outplanes, stride=1, res_conv=False, groups=1, drop_block=None, drop_path=None,
                 conv_cfg=dict(type="DynConv2d"), norm_cfg=dict(type="DynBN", requires_grad=True),
                 act_cfg=dict(type="ReLU", inplace=True)):
        super().__init__()
        if groups != 1 or drop_block is not None or drop_path is not None:
            raise NotImplementedError("Elastic_conv_Block: groups / drop_block / drop_path are not used by "
                                      "ElasticConvformer")
        self.expansion = EXPANSION
        med_planes = _check_width(outplanes) // self.expansion
        self.conv1 = build_conv_layer(conv_cfg, inplanes, med_planes, kernel_size=1, stride=1, padding=0,
                                      bias=False)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, med_planes, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.act1 = build_activation_layer(act_cfg)
        self.conv2 = build_conv_layer(conv_cfg, med_planes, med_planes, kernel_size=3, stride=stride,
                                      groups=groups, padding=1, bias=False)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, med_planes, postfix=2)
        self.add_module(self.norm2_name, norm2)
        self.act2 = build_activation_layer(act_cfg)
        self.conv3 = build_conv_layer(conv_cfg, med_planes, outplanes, kernel_size=1, stride=1, padding=0,
                                      bias=False)
        self.norm3_name, norm3 = build_norm_layer(norm_cfg, outplanes, postfix=3)
        self.add_module(self.norm3_name, norm3)
        self.act3 = build_activation_layer(act_cfg)
        if res_conv:
            self.residual_conv = build_conv_layer(conv_cfg, inplanes, outplanes, kernel_size=1, stride=stride,
                                                  padding=0, bias=False)
            self.norm4_name, norm4 = build_norm_layer(norm_cfg, outplanes, postfix=4)
            self.add_module(self.norm4_name, norm4)
        self.res_conv, self.drop_block, self.drop_path = res_conv, drop_block, drop_path
        self.init_state(width=outplanes)

    norm1 = property(lambda self: getattr(self, self.norm1_name))
    norm2 = property(lambda self: getattr(self, self.norm2_name))
    norm3 = property(lambda self: getattr(self, self.norm3_name))
    norm4 = property(lambda self: getattr(self, self.norm4_name))

    def zero_init_last_bn(self):
        nn.init.zeros_(self.norm3.weight)

    def manipulate_width(self, arch_meta):
        self.width_state = _check_width(arch_meta)
        self.conv1.manipulate_width(arch_meta // self.expansion)
        self.conv2.manipulate_width(arch_meta // self.expansion)
        self.conv3.manipulate_width(arch_meta)
        if self.res_conv:
            self.residual_conv.manipulate_width(arch_meta)

    def forward_act(self, tape, x, x_t=None, up_stride=1):
        """-> (block output, x2 = the 3x3 conv's activated output, what the conv-to-token unit reads)"""
        out = conv_bn_act(tape, self.conv1, self.norm1, x, relu=True)
        if x_t is not None:
            out = ops.fcu_up_add(tape, out, x_t, up_stride)
        x2 = conv_bn_act(tape, self.conv2, self.norm2, out, relu=True)
        residual = x
        if self.res_conv:
            residual = conv_bn_act(tape, self.residual_conv, self.norm4, x, relu=False)
        return conv_bn_act(tape, self.conv3, self.norm3, x2, relu=True, residual=residual), x2


class Elastic_conv2trans(nn.Module, DynamicMixin):
    """CNN feature maps -> transformer patch embeddings, added to the token stream"""

    def __init__(self, inplanes, outplanes, dw_stride, conv_cfg=dict(type="DynConv2d"),
                 norm_cfg=dict(type="ElaLN"), act_cfg=dict(type="GELU")):
        super().__init__()
        self.dw_stride = dw_stride
        self.conv_project = build_conv_layer(conv_cfg, inplanes, outplanes, kernel_size=1, stride=1, padding=0)
        self.sample_pooling = nn.AvgPool2d(kernel_size=dw_stride, stride=dw_stride)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, outplanes, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.act = build_activation_layer(act_cfg)

    norm1 = property(lambda self: getattr(self, self.norm1_name))

    def forward_act(self, tape, x, x_t):
        """x_t + cat(x_t[:, :1], GELU(LN(pool(conv_project(x))))), the pooling moved in front of the conv"""
        if x.H % self.dw_stride or x.W % self.dw_stride:
            raise ValueError("img_size: a %d x %d map has no whole %d x %d pooling windows"
                             % (x.H, x.W, self.dw_stride, self.dw_stride))
        if self.dw_stride > 1:
            x = ops.avgpool_ceil(tape, x, self.dw_stride)
        norm = self.norm1
        z = self.conv_project.forward_act(tape, x)
        if getattr(norm, "_deploying", False):
            norm._deploy_slice(z.C)
        return ops.fcu_down(tape, z, x_t, norm)


class Elastic_trans2conv(nn.Module, DynamicMixin):
    """Transformer patch embeddings -> CNN feature maps (at the token grid's size: the upsample is the
    consumer's, ops.fcu_up_add)"""

    def __init__(self, inplanes, outplanes, up_stride, conv_cfg=dict(type="DynConv2d"),
                 norm_cfg=dict(type="DynBN", requires_grad=True), act_cfg=dict(type="ReLU")):
        super().__init__()
        self.up_stride = up_stride
        self.conv_project = build_conv_layer(conv_cfg, inplanes, outplanes, kernel_size=1, stride=1, padding=0)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, outplanes, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.act = build_activation_layer(act_cfg)

    norm1 = property(lambda self: getattr(self, self.norm1_name))

    def forward_act(self, tape, x_t, h, w):
        x_r = ops.vit_feature_map(tape, x_t, h, w)
        return conv_bn_act(tape, self.conv_project, self.norm1, x_r, relu=True)


class Elastic_ConvTrans_Block(nn.Module, DynamicMixin):
    """One block of both branches.  ``stage`` true: the first block of the network (a bottleneck, the patch
    embedding and a transformer block, no coupling); else conv block, conv-to-token unit, transformer block,
    token-to-conv unit and the fusion conv block."""
    search_space = {"convblock", "embed_dim", "transblock"}

    def __init__(self, inplanes, outplanes, stage, res_conv, stride, dw_stride, embed_dim, num_heads, mlp_ratio,
                 proj_drop=0., attn_drop=0., drop_path=0., last_fusion=False, groups=1,
                 conv_cfg=dict(type="DynConv2d"), relative_position=False):
        super().__init__()
        self.stage = stage
        trans = dict(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, proj_drop=proj_drop,
                     attn_drop=attn_drop, drop_path=drop_path, relative_position=relative_position)
        if stage:
            self.conv_1 = Elastic_conv_Block(inplanes=inplanes, outplanes=outplanes, res_conv=True, stride=1)
            self.trans_patch_conv = build_conv_layer(conv_cfg, inplanes, embed_dim, kernel_size=dw_stride,
                                                     stride=dw_stride, padding=0)
            self.trans_1 = Elastic_trans_Block(**trans)
        else:
            self.cnn_block = Elastic_conv_Block(inplanes=inplanes, outplanes=outplanes, res_conv=res_conv,
                                                stride=stride, groups=groups)
            if last_fusion:
                self.fusion_block = Elastic_conv_Block(inplanes=outplanes, outplanes=outplanes, stride=2,
                                                       res_conv=True, groups=groups)
            else:
                self.fusion_block = Elastic_conv_Block(inplanes=outplanes, outplanes=outplanes, groups=groups)
            self.squeeze_block = Elastic_conv2trans(inplanes=outplanes // EXPANSION, outplanes=embed_dim,
                                                    dw_stride=dw_stride)
            self.expand_block = Elastic_trans2conv(inplanes=embed_dim, outplanes=outplanes // EXPANSION,
                                                   up_stride=dw_stride)
            self.trans_block = Elastic_trans_Block(**trans)
            self.dw_stride, self.embed_dim = dw_stride, embed_dim
            self.last_fusion, self.expansion = last_fusion, EXPANSION

    transformer = property(lambda self: self.trans_1 if self.stage else self.trans_block)

    def manipulate_convblock(self, arch_meta):
        if self.stage:
            self.conv_1.manipulate_arch(arch_meta)
        else:
            self.cnn_block.manipulate_arch(arch_meta)
            self.fusion_block.manipulate_arch(arch_meta)
            self.expand_block.conv_project.manipulate_arch({"width": arch_meta["width"] // EXPANSION})

    def manipulate_embed_dim(self, arch_meta):
        d = arch_meta["width"]
        if d % 4 or d <= 0:
            raise ValueError("embed_dim: the width %s is no positive multiple of 4" % d)
        self.embed_dim = d
        (self.trans_patch_conv if self.stage else self.squeeze_block.conv_project).manipulate_arch(arch_meta)
        self.transformer.manipulate_arch(arch_meta)

    def manipulate_transblock(self, arch_meta):
        self.transformer.manipulate_arch(arch_meta)

    def active_children(self):
        """the modules of this block that hold parameters the forward reads"""
        if self.stage:
            return [self.conv_1, self.trans_patch_conv] + self.trans_1.active_children()
        return [self.cnn_block, self.fusion_block, self.squeeze_block.conv_project, self.squeeze_block.norm1,
                self.expand_block.conv_project, self.expand_block.norm1] + self.trans_block.active_children()

    def forward_act(self, tape, x, x_t=None, cls_token=None):
        if self.stage:
            x_base = x
            x, _ = self.conv_1.forward_act(tape, x_base)
            x_t = ops.fcu_tokens(tape, self.trans_patch_conv.forward_act(tape, x_base), cls_token)
            return x, self.trans_1.forward_act(tape, x_t)
        x, x2 = self.cnn_block.forward_act(tape, x)
        x_t = self.trans_block.forward_act(tape, self.squeeze_block.forward_act(tape, x2, x_t))
        x_t_r = self.expand_block.forward_act(tape, x_t, x2.H // self.dw_stride, x2.W // self.dw_stride)
        x, _ = self.fusion_block.forward_act(tape, x, x_t_r, self.dw_stride)
        return x, x_t


class Elastic_Block(nn.ModuleList, DynamicMixin):
    """One stage: ``depth`` blocks at their maximum size, only the first ``depth_state`` run."""
    search_space = {"depth", "block"}

    def init_state(self, depth=None, block=None, **kwargs):
        if depth is not None:
            self.depth_state = depth
        if block is not None:
            self.block_state = block
        for k, v in kwargs.items():
            setattr(self, "%s_state" % k, v)

    def __init__(self, inplanes, outplanes, depth, stage, dw_stride, embed_dim, num_heads, mlp_ratio, proj_drop=0.,
                 attn_drop=0., drop_path=0., last_fusion=False, groups=1, relative_position=False):
        blocks = []
        for i in range(depth):
            first = stage == 1 and i == 0
            blocks.append(Elastic_ConvTrans_Block(
                inplanes=inplanes if stage == 4 else inplanes[0 if i == 0 else 1], outplanes=outplanes,
                stage=first, res_conv=i == 0 and stage != 4, stride=2 if (stage in (2, 3) and i == 0) else 1,
                dw_stride=dw_stride, embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio,
                proj_drop=proj_drop, attn_drop=attn_drop, drop_path=drop_path if stage == 4 else drop_path[i],
                last_fusion=last_fusion, groups=groups, relative_position=relative_position))
        super().__init__(blocks)
        self.depth_state = depth

    def manipulate_depth(self, arch_meta):
        assert arch_meta >= 1, "Depth must be greater than 0, skipping stage is not supported yet."
        if arch_meta > len(self):
            raise ValueError("depth %d exceeds the %d blocks of this stage" % (arch_meta, len(self)))
        self.depth_state = arch_meta

    def manipulate_block(self, arch_meta):
        self.arch_meta = arch_meta
        for m in self:   # every block, skipped ones included, as in the reference
            m.manipulate_arch(arch_meta)

    def active_blocks(self):
        return [self[i] for i in range(self.depth_state)]

    def forward_act(self, tape, x, x_t=None, cls_token=None):
        if getattr(self, "_deploying", False):
            del self[self.depth_state:]
        for i in range(self.depth_state):
            x, x_t = self[i].forward_act(tape, x, x_t, cls_token)
        return x, x_t


@BACKBONES.register_module()
class ElasticConvformer(nn.Module, DynamicMixin):
    """Conformer with an elastic stem width and, per stage, elastic depth, conv width, head count and
    feed-forward ratio, and an elastic embedding width."""
    search_space = {"stem", "body"}
    _fp16_attention = False

    def init_state(self, stem=None, body=None, **kwargs):
        if stem is not None:
            self.stem_state = stem
        if body is not None:
            self.body_state = body
        for k, v in kwargs.items():
            setattr(self, "%s_state" % k, v)

    def __init__(self, embed_dim, num_heads, mlp_ratio, depth, stem_width, body_width, body_depth, patch_size=16,
                 in_chans=3, proj_drop=0., attn_drop=0., drop_path=0.1, conv_cfg=dict(type="DynConv2d"),
                 norm_cfg=dict(type="DynBN", requires_grad=True), act_cfg=dict(type="ReLU", inplace=True),
                 pretrained=None, init_cfg=None, relative_position=False, norm_eval=True):
        super().__init__()
        assert not (init_cfg and pretrained), "init_cfg and pretrained cannot be setting at the same time"
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        _refuse_positive(drop_path=drop_path, attn_drop=attn_drop, proj_drop=proj_drop)
        if relative_position:
            raise NotImplementedError("relative_position=True is not implemented (the reference never turns "
                                      "it on)")
        if patch_size not in (16, 32):
            raise NotImplementedError("patch_size %r: 16 or 32 (the strides patch_size / 4, / 8, / 16 of the "
                                      "coupling units must be whole)" % (patch_size,))
        if len(body_width) != 3 or len(body_depth) != 3 or len(num_heads) != 3 or len(mlp_ratio) != 3:
            raise AssertionError("ElasticConvformer has three searched stages: body_width, body_depth, "
                                 "num_heads and mlp_ratio need three entries")
        if depth % 3:
            raise ValueError("depth %d must be a multiple of 3" % depth)
        if depth <= sum(body_depth):
            raise ValueError("depth %d must exceed sum(body_depth) = %d: stage 4 takes the drop-path rate of "
                             "block sum(body_depth)" % (depth, sum(body_depth)))
        for w in body_width:
            _check_width(w, "body_width")
        self.pretrained, self.init_cfg = pretrained, init_cfg
        self.embed_dim, self.num_heads, self.mlp_ratio = embed_dim, list(num_heads), list(mlp_ratio)
        self.depth, self.stem_width, self.patch_size = depth, stem_width, patch_size
        self.body_width, self.body_depth = list(body_width), list(body_depth)
        self.norm_eval = norm_eval
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.init_state(stem={"width": stem_width},
                        body={"depth": body_depth,
                              "block": {"convblock": {"width": body_width},
                                        "embed_dim": {"width": embed_dim},
                                        "transblock": {"MHA": _nest("num_heads", tuple(num_heads)),
                                                       "FFN": _nest("feedforward_channels", tuple(mlp_ratio))}}})
        self.conv1 = build_conv_layer(conv_cfg, in_chans, stem_width, kernel_size=7, stride=2, padding=3,
                                      bias=False)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, stem_width, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.act1 = build_activation_layer(act_cfg)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        trans_dw_stride = patch_size // 4
        dw_stride = [trans_dw_stride, trans_dw_stride // 2, trans_dw_stride // 4]
        self.layers = []
        inplanes = [stem_width, body_width[0]]
        for i, num_blocks in enumerate(self.body_depth):
            name = "conv_trans_%d" % (i + 1)
            self.add_module(name, self.make_layer(
                inplanes=inplanes, outplanes=body_width[i], depth=num_blocks, stage=i + 1, dw_stride=dw_stride[i],
                embed_dim=embed_dim, num_heads=num_heads[i], mlp_ratio=mlp_ratio[i], proj_drop=0., attn_drop=0.,
                drop_path=[0.] * num_blocks, last_fusion=False, groups=1))
            if i < 2:
                inplanes = [body_width[i], body_width[i + 1]]
            self.layers.append(name)
        self.add_module("conv_trans_4", self.make_layer(
            inplanes=body_width[2], outplanes=body_width[2], depth=1, stage=4, dw_stride=dw_stride[2],
            embed_dim=embed_dim, num_heads=num_heads[2], mlp_ratio=mlp_ratio[2], proj_drop=0., attn_drop=0.,
            drop_path=0., last_fusion=True, groups=1, relative_position=relative_position))
        self.layers.append("conv_trans_4")
        self.init_weights()

    norm1 = property(lambda self: getattr(self, self.norm1_name))

    @property
    def fp16_attention(self):
        """Opt-in, as on ElasticTransformer (core.fp16_utils.wrap_fp16_model(model, attention=True)): inside
        an fp16 mode every attention runs on the fp16-operand kernels.  Without an fp16 mode the flag does
        nothing."""
        return self._fp16_attention

    @fp16_attention.setter
    def fp16_attention(self, flag):
        self._fp16_attention = bool(flag)
        for m in self.modules():
            if isinstance(m, ElasticMHA):
                m.fp16_attention = self._fp16_attention

    def make_layer(self, **kwargs):
        return Elastic_Block(**kwargs)

    def init_weights(self, pretrained=None):
        """The reference's ``_init_weights``: normal (std 0.02) linears with zero biases and cls token, unit
        LayerNorms and BatchNorms, He-normal (fan-out) convs; then the checkpoint, if a path is given (here,
        as the segmentor does, or to the constructor)."""
        if pretrained is not None:
            if not isinstance(pretrained, str):
                raise TypeError("pretrained must be a str or None")
            self.pretrained = pretrained
        nn.init.normal_(self.cls_token, std=0.02)
        for m in self.modules():
            if isinstance(m, DynamicLinear):
                nn.init.normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, DynamicConv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.LayerNorm, _BatchNorm)):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)
        if isinstance(self.pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, self.pretrained, strict=False)

    def _freeze_stages(self):
        freeze(self.norm1)
        for p in self.conv1.parameters():
            p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:   # BatchNorm keeps its running statistics while training
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self

    # ---- arch manipulation ----
    def manipulate_stem(self, arch_meta):
        self.stem_state = arch_meta
        self.conv1.manipulate_arch(arch_meta)

    def manipulate_body(self, arch_meta):
        """One entry of depth, width, heads and ratio per searched stage; stage 4 runs its one block at stage
        3's width, heads and ratio.  The meta is only read."""
        self.body_state = arch_meta
        block = arch_meta["block"]
        widths, d = block["convblock"]["width"], block["embed_dim"]["width"]
        heads = _leaf(block["transblock"]["MHA"], "num_heads")
        ratios = _leaf(block["transblock"]["FFN"], "feedforward_channels")
        for i, name in enumerate(self.layers):
            j = min(i, 2)
            getattr(self, name).manipulate_arch({
                "depth": arch_meta["depth"][i] if i < 3 else 1,
                "block": {"convblock": {"width": widths[j]}, "embed_dim": {"width": d},
                          "transblock": {"MHA": _nest("num_heads", heads[j]),
                                         "FFN": _nest("feedforward_channels", ratios[j])}}})

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        ratios = [round(10 * r) for r in self.mlp_ratio]
        for r, m in zip(ratios, self.mlp_ratio):
            if ffn_width(r, self.embed_dim) != int(self.embed_dim * m):
                raise ValueError("mlp_ratio %s is not a whole number of tenths of embed_dim %d"
                                 % (m, self.embed_dim))
        return {"stem": {"width": self.stem_width},
                "body": {"depth": list(self.body_depth),
                         "block": {"convblock": {"width": list(self.body_width)},
                                   "embed_dim": {"width": self.embed_dim},
                                   "transblock": {"MHA": _nest("num_heads", list(self.num_heads)),
                                                  "FFN": _nest("feedforward_channels", ratios)}}}}

    # ---- execution ----
    def forward_act(self, tape, img):
        h, w = (img.t.shape[2], img.t.shape[3]) if img.nchw_image else (img.H, img.W)
        if h % (2 * self.patch_size) or w % (2 * self.patch_size):
            raise ValueError("img_size: the input (%d*%d) must be a multiple of 2 * patch_size = %d in both "
                             "directions" % (h, w, 2 * self.patch_size))
        x = conv_bn_act(tape, self.conv1, self.norm1, img, relu=True)
        mp = self.maxpool
        x = ops.maxpool(tape, x, mp.kernel_size, mp.stride, mp.padding)
        d = self.conv_trans_1[0].trans_patch_conv.width_state
        if getattr(self, "_deploying", False) and self.cls_token.shape[-1] != d:
            self.cls_token = nn.Parameter(self.cls_token.data[..., :d].clone(), self.cls_token.requires_grad)
        outs, x_t = [], None
        for i, name in enumerate(self.layers):
            x, x_t = getattr(self, name).forward_act(tape, x, x_t, self.cls_token)
            if i == 0:
                streams.side_checkpoint(tape)   # as the other backbones: later layers' gradients are ready first
            outs.append(x)
        return outs

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (stem, cls token,
        stage 1)."""
        params = [self.cls_token] + list(self.conv1.parameters()) + list(self.norm1.parameters())
        for block in self.conv_trans_1.active_blocks():
            params += [p for m in block.active_children() for p in m.parameters()]
        return params

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: the stem, the cls token and, of the
        blocks the depth states keep, the conv blocks, projections, norms and linears; not the skipped
        blocks or the relative-position tables."""
        mods = [self.conv1, self.norm1, _ClsToken(self)]
        for name in self.layers:
            for block in getattr(self, name).active_blocks():
                mods.extend(block.active_children())
        return mods


class _ClsToken:
    """cls_token as a 'module' of active_modules(): it is a parameter of the backbone itself, whose unused
    children must not come along."""

    def __init__(self, backbone):
        self._params = [backbone.cls_token]

    def parameters(self):
        return iter(self._params)
