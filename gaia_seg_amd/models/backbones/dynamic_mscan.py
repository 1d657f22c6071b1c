"""DynamicMSCAN backbone: SegNeXt's multi-scale convolutional attention network (MSCAN, Guo et al., NeurIPS
2022) as a supernet.

Constructor, module and parameter names are those of mmseg's ``MSCAN`` (``patch_embed1.proj.{0,1,3,4}``,
``patch_embed{2..4}.{proj,norm}``, ``block{i}.{j}.{norm1, attn.proj_1, attn.spatial_gating_unit.conv0,
conv0_1, conv0_2, conv1_1, conv1_2, conv2_1, conv2_2, conv3, attn.proj_2, norm2, mlp.fc1, mlp.dwconv, mlp.fc2,
layer_scale_1, layer_scale_2}``, ``norm{i}``), so an mmseg MSCAN state dict loads with ``strict=True`` into a
DynamicMSCAN built at that size.  MSCAN-T / S / B differ in depth, width and feed-forward ratio per stage
only; the supernet is elastic in exactly those: search-space key ``body`` = {"depth": [4], "width": [4],
"mlp_ratio": [4]}, leading slices of every parameter, the next stage's patch embedding follows the width of
the stage that feeds it, only the first depth[i] blocks of a stage run.  Metas are only read.

``forward`` returns logical NCHW feature maps and runs the whole backbone as ONE autograd node over
hand-written HIP kernels, NHWC throughout.  A block computes, with sgu = attn.spatial_gating_unit,

    n1 = norm1(x)                                              BatchNorm
    u  = GELU(attn.proj_1(n1))
    s  = a + sum_i sgu.conv{i}_2(sgu.conv{i}_1(a)),  a = sgu.conv0(u)   depthwise 5x5, then 1xK + Kx1 pairs
    g  = sgu.conv3(s) * u
    x  = x + layer_scale_1 * (attn.proj_2(g) + n1)             (the inner shortcut is n1, not x)
    x  = x + layer_scale_2 * mlp.fc2(GELU(mlp.dwconv(mlp.fc1(norm2(x)))))

with the seven depthwise filters of the spatial gating unit as ONE operator (ops.msca on csrc/msca.hip), the
gate on ops.gate_mul, the 1x1 and the patch-embedding convolutions on gs_conv2d_*, the feed-forward's
depthwise 3x3 on gs_dwconv2d_*, BatchNorm, LayerNorm, GELU and the layer-scaled residual on the kernels
the other backbones use.  x feeds both a BatchNorm, whose backward has no accumulate form, and the
residual: the BatchNorm reads an alias of x whose gradient is added to x's afterwards.

Refused: ``drop_path_rate`` and ``drop_rate > 0`` (stochastic depth and dropout are not implemented),
``num_stages != 4``, an ``act_cfg`` other than the exact GELU, ``attention_kernel_sizes`` other than one
odd square K0 <= 7 plus three [1, K] strips with odd K <= 21, paddings that are not "same"; widths that are
not multiples of 4 (8 in stage 1: the stem runs at half the width) and hidden widths int(ratio * width) that
are no multiple of 4.  Out of scope: SegNeXt's LightHamHead, converters for the original repository's
checkpoint keys.
"""
import math

import torch
import torch.nn as nn

from ...core.bricks import (DynamicConv2d, DynamicDepthwiseConv2d, DynamicLayerNorm, GELU, build_norm_layer,
                            conv_bn_act)
from ...core.dynamic import DynamicMixin, unzip_meta
from ...hip import ops, streams
from ...hip.runtime import Act, tape_function
from ..builder import BACKBONES


def _refuse_positive(**kwargs):
    for key, value in kwargs.items():
        if value and value > 0:
            raise NotImplementedError("%s > 0 is not implemented (set %s=0)" % (key, key))


def hidden_width(mlp_ratio, width):
    """hidden width of the feed-forward (mmseg's MSCABlock: int(channels * mlp_ratio))"""
    return int(mlp_ratio * width)


def check_widths(stage, width, mlp_ratio, what="body"):
    """What the kernels need of stage ``stage`` (0-based): float4 channel quads everywhere."""
    if not isinstance(width, int) or width <= 0 or width % 4:
        raise ValueError("%s.width: stage %d width %s is no positive multiple of 4" % (what, stage + 1, width))
    if stage == 0 and width % 8:
        raise ValueError("%s.width: stage 1 width %d is no multiple of 8 (the stem runs at half of it)"
                         % (what, width))
    hidden = hidden_width(mlp_ratio, width)
    if hidden <= 0 or hidden % 4:
        raise ValueError("%s.mlp_ratio: stage %d hidden width int(%s * %d) = %d is no positive multiple of 4"
                         % (what, stage + 1, mlp_ratio, width, hidden))


def _branch_input(tape, x):
    """``x`` for a consumer whose backward only writes a fresh gradient (BatchNorm) while x also feeds a
    residual edge: an alias whose gradient is added to x's once that consumer's backward has run."""
    alias = Act(x.t, x.requires_grad)
    ops.add_grad_passthrough(tape, x, alias)
    return alias


class StemConv(nn.Module):
    """mmseg's StemConv: 3x3 s2 conv to half the width, BN, GELU, 3x3 s2 conv, BN"""

    def __init__(self, in_channels, width, norm_cfg):
        super().__init__()
        self.proj = nn.Sequential(
            DynamicConv2d(in_channels, width // 2, 3, stride=2, padding=1),
            build_norm_layer(norm_cfg, width // 2)[1],
            GELU(),
            DynamicConv2d(width // 2, width, 3, stride=2, padding=1),
            build_norm_layer(norm_cfg, width)[1])

    def manipulate_width(self, width):
        self.proj[0].manipulate_width(width // 2)
        self.proj[3].manipulate_width(width)

    def forward_act(self, tape, x):
        x = conv_bn_act(tape, self.proj[0], self.proj[1], x)
        x = self.proj[2].forward_act(tape, x)
        return conv_bn_act(tape, self.proj[3], self.proj[4], x)


class OverlapPatchEmbed(nn.Module):
    """mmseg's OverlapPatchEmbed: 3x3 s2 conv, BN"""

    def __init__(self, in_channels, width, norm_cfg):
        super().__init__()
        self.proj = DynamicConv2d(in_channels, width, 3, stride=2, padding=1)
        self.norm = build_norm_layer(norm_cfg, width)[1]

    def manipulate_width(self, width):
        self.proj.manipulate_width(width)

    def forward_act(self, tape, x):
        return conv_bn_act(tape, self.proj, self.norm, x)


class MSCAAttention(nn.Module, DynamicMixin):
    """the spatial gating unit: conv3(a + sum of the three strip pairs of a) * u, a = conv0(u)"""
    search_space = set()

    def __init__(self, channels, kernel_sizes, paddings):
        super().__init__()
        self.conv0 = DynamicDepthwiseConv2d(channels, kernel_sizes[0], paddings[0])
        for i, (ks, pad) in enumerate(zip(kernel_sizes[1:], paddings[1:])):
            self.add_module("conv%d_1" % i, DynamicDepthwiseConv2d(channels, tuple(ks), tuple(pad)))
            self.add_module("conv%d_2" % i, DynamicDepthwiseConv2d(channels, tuple(ks)[::-1], tuple(pad)[::-1]))
        self.conv3 = DynamicConv2d(channels, channels, 1)

    def depthwise(self):
        rows = [getattr(self, "conv%d_1" % i) for i in range(3)]
        cols = [getattr(self, "conv%d_2" % i) for i in range(3)]
        return [self.conv0] + rows + cols

    def filters(self):
        """the 14 parameters in the order of gs_msca_filters"""
        dw = self.depthwise()
        rows, cols = dw[1:4], dw[4:7]
        return ([self.conv0.weight, self.conv0.bias] + [m.weight for m in rows] + [m.bias for m in rows]
                + [m.weight for m in cols] + [m.bias for m in cols])

    def manipulate_width(self, width):
        for m in self.depthwise():
            m.manipulate_width(width)
        self.conv3.manipulate_width(width)

    def prune(self, width):
        for m in self.depthwise():
            m._deploy_slice(width)
        self.conv3._deploy_slice(width)

    def forward_act(self, tape, u):
        for m in self.depthwise():
            m.check_layout()
        s = ops.msca(tape, u, self)
        return ops.gate_mul(tape, self.conv3.forward_act(tape, s), u)


class MSCASpatialAttention(nn.Module):
    """proj_2(sgu(GELU(proj_1(n1)))) + n1"""

    def __init__(self, channels, kernel_sizes, paddings):
        super().__init__()
        self.proj_1 = DynamicConv2d(channels, channels, 1)
        self.activation = GELU()
        self.spatial_gating_unit = MSCAAttention(channels, kernel_sizes, paddings)
        self.proj_2 = DynamicConv2d(channels, channels, 1)

    def manipulate_width(self, width):
        self.proj_1.manipulate_width(width)
        self.spatial_gating_unit.manipulate_width(width)
        self.proj_2.manipulate_width(width)

    def forward_act(self, tape, n1):
        u = self.activation.forward_act(tape, self.proj_1.forward_act(tape, n1))
        g = self.spatial_gating_unit.forward_act(tape, u)
        return ops.layer_scale_add(tape, n1, self.proj_2.forward_act(tape, g), None)


class MSCAMlp(nn.Module):
    """fc2(GELU(dwconv3x3(fc1(x)))), 1x1 convolutions with 4-D weights"""

    def __init__(self, channels, hidden):
        super().__init__()
        self.fc1 = DynamicConv2d(channels, hidden, 1)
        self.dwconv = DynamicConv2d(hidden, hidden, 3, padding=1, groups=hidden)
        self.act = GELU()
        self.fc2 = DynamicConv2d(hidden, channels, 1)

    def manipulate(self, width, hidden):
        self.fc1.manipulate_width(hidden)
        self.dwconv.manipulate_width(hidden)
        self.fc2.manipulate_width(width)

    def forward_act(self, tape, x):
        z = self.fc1.forward_act(tape, x)
        z = self.dwconv.forward_act(tape, z)
        z = self.act.forward_act(tape, z)
        return self.fc2.forward_act(tape, z)


class MSCABlock(nn.Module, DynamicMixin):
    search_space = set()

    def __init__(self, channels, kernel_sizes, paddings, mlp_ratio, norm_cfg):
        super().__init__()
        self.norm1 = build_norm_layer(norm_cfg, channels)[1]
        self.attn = MSCASpatialAttention(channels, kernel_sizes, paddings)
        self.norm2 = build_norm_layer(norm_cfg, channels)[1]
        self.mlp = MSCAMlp(channels, hidden_width(mlp_ratio, channels))
        self.layer_scale_1 = nn.Parameter(1e-2 * torch.ones(channels))
        self.layer_scale_2 = nn.Parameter(1e-2 * torch.ones(channels))

    def manipulate(self, width, hidden):
        self.attn.manipulate_width(width)
        self.mlp.manipulate(width, hidden)

    def prune(self, width, hidden):
        """Physically cut every parameter to ``width`` channels and ``hidden`` hidden channels."""
        self.norm1._deploy_slice(width)
        self.norm2._deploy_slice(width)
        self.attn.proj_1._deploy_slice(width)
        self.attn.spatial_gating_unit.prune(width)
        self.attn.proj_2._deploy_slice(width)
        self.mlp.fc1._deploy_slice(width)
        self.mlp.dwconv._deploy_slice(hidden)
        self.mlp.fc2._deploy_slice(hidden)
        if self.layer_scale_1.numel() != width:
            for name in ("layer_scale_1", "layer_scale_2"):
                p = getattr(self, name)
                setattr(self, name, nn.Parameter(p.data[:width].clone(), p.requires_grad))

    def forward_act(self, tape, x):
        n1 = self.norm1.forward_act(tape, _branch_input(tape, x))
        x = ops.layer_scale_add(tape, x, self.attn.forward_act(tape, n1), self.layer_scale_1)
        z = self.mlp.forward_act(tape, self.norm2.forward_act(tape, _branch_input(tape, x)))
        return ops.layer_scale_add(tape, x, z, self.layer_scale_2)


def _check_attention_kernels(sizes, paddings):
    """one odd square K0 <= 7 and three [1, K] strips with odd K <= 21, "same" paddings"""
    sizes, paddings = list(sizes), list(paddings)
    ok = len(sizes) == 4 and isinstance(sizes[0], int) and sizes[0] % 2 == 1 and 1 <= sizes[0] <= 7
    ok = ok and all(isinstance(s, (list, tuple)) and len(s) == 2 and s[0] == 1 and isinstance(s[1], int)
                    and s[1] % 2 == 1 and 1 <= s[1] <= 21 for s in sizes[1:])
    if not ok:
        raise NotImplementedError("attention_kernel_sizes %s: one odd square size <= 7 and three [1, K] strips "
                                  "with odd K <= 21 are what the msca kernels run" % (sizes,))
    same = len(paddings) == 4 and paddings[0] == sizes[0] // 2 and all(
        isinstance(p, (list, tuple)) and list(p) == [0, s[1] // 2] for p, s in zip(paddings[1:], sizes[1:]))
    if not same:
        raise NotImplementedError("attention_kernel_paddings %s: only \"same\" paddings (K // 2) of "
                                  "attention_kernel_sizes %s are implemented" % (paddings, sizes))


@BACKBONES.register_module()
class DynamicMSCAN(nn.Module, DynamicMixin):
    """SegNeXt's MSCAN encoder with, per stage, elastic depth, width and feed-forward ratio."""
    search_space = {"body"}

    def __init__(self, in_channels=3, embed_dims=(64, 128, 320, 512), mlp_ratios=(8, 8, 4, 4),
                 depths=(3, 3, 12, 3), num_stages=4, drop_rate=0., drop_path_rate=0.,
                 attention_kernel_sizes=(5, (1, 7), (1, 11), (1, 21)),
                 attention_kernel_paddings=(2, (0, 3), (0, 5), (0, 10)), act_cfg=dict(type="GELU"),
                 norm_cfg=dict(type="SyncBN", requires_grad=True), out_indices=(0, 1, 2, 3), pretrained=None):
        super().__init__()
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        _refuse_positive(drop_path_rate=drop_path_rate, drop_rate=drop_rate)
        if num_stages != 4:
            raise NotImplementedError("num_stages: MSCAN has four stages")
        if dict(act_cfg) != dict(type="GELU") and dict(act_cfg) != dict(type="GELU", approximate="none"):
            raise NotImplementedError("act_cfg %s: the exact GELU (type 'GELU') is the only activation of MSCAN"
                                      % (act_cfg,))
        _check_attention_kernels(attention_kernel_sizes, attention_kernel_paddings)
        for key, value in (("embed_dims", embed_dims), ("mlp_ratios", mlp_ratios), ("depths", depths)):
            if len(value) != 4:
                raise ValueError("%s needs four entries, one per stage (got %s)" % (key, (value,)))
        for i in range(4):
            check_widths(i, embed_dims[i], mlp_ratios[i], "embed_dims / mlp_ratios")
        self.embed_dims, self.mlp_ratios, self.depths = list(embed_dims), list(mlp_ratios), list(depths)
        self.num_stages, self.out_indices = 4, list(out_indices)
        self.init_state(body=self.full_arch_meta()["body"])
        sizes = [attention_kernel_sizes[0]] + [tuple(s) for s in attention_kernel_sizes[1:]]
        pads = [attention_kernel_paddings[0]] + [tuple(p) for p in attention_kernel_paddings[1:]]
        ci = in_channels
        for i, width in enumerate(self.embed_dims):
            embed = StemConv(ci, width, norm_cfg) if i == 0 else OverlapPatchEmbed(ci, width, norm_cfg)
            self.add_module("patch_embed%d" % (i + 1), embed)
            self.add_module("block%d" % (i + 1), nn.ModuleList(
                [MSCABlock(width, sizes, pads, self.mlp_ratios[i], norm_cfg) for _ in range(self.depths[i])]))
            self.add_module("norm%d" % (i + 1), DynamicLayerNorm(width, eps=1e-5))
            ci = width
        self.init_weights(pretrained)

    def stage(self, i):
        """(patch embedding, blocks, norm) of stage i (0-based)"""
        return (getattr(self, "patch_embed%d" % (i + 1)), getattr(self, "block%d" % (i + 1)),
                getattr(self, "norm%d" % (i + 1)))

    def init_weights(self, pretrained=None):
        """mmseg's MSCAN init: fan-out normal convs, zero biases, unit LayerNorms; then the checkpoint, if a
        path is given."""
        for m in self.modules():
            if isinstance(m, (DynamicConv2d, DynamicDepthwiseConv2d)):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0, math.sqrt(2.0 / fan_out))
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)
        if isinstance(pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)

    # ---- arch manipulation ----
    def manipulate_body(self, arch_meta):
        """{'depth': [d1..d4], 'width': [w1..w4], 'mlp_ratio': [r1..r4]}: one entry per stage; the next
        stage's patch embedding follows the width of the stage that feeds it.  The meta is only read."""
        for key in ("depth", "width", "mlp_ratio"):
            if key not in arch_meta or len(arch_meta[key]) != 4:
                raise ValueError("body.%s: four entries, one per stage (got %s)" % (key, arch_meta.get(key)))
        metas = unzip_meta({k: arch_meta[k] for k in ("depth", "width", "mlp_ratio")})
        for i, meta in enumerate(metas):
            if not (isinstance(meta["depth"], int) and 1 <= meta["depth"] <= self.depths[i]):
                raise ValueError("body.depth: stage %d depth %s out of range (1..%d)"
                                 % (i + 1, meta["depth"], self.depths[i]))
            if not (isinstance(meta["width"], int) and 0 < meta["width"] <= self.embed_dims[i]):
                raise ValueError("body.width: stage %d width %s out of range (1..%d)"
                                 % (i + 1, meta["width"], self.embed_dims[i]))
            if not 0 < meta["mlp_ratio"] <= self.mlp_ratios[i]:
                raise ValueError("body.mlp_ratio: stage %d ratio %s out of range (0..%s]"
                                 % (i + 1, meta["mlp_ratio"], self.mlp_ratios[i]))
            check_widths(i, meta["width"], meta["mlp_ratio"])
        self.body_state = arch_meta
        for i, meta in enumerate(metas):
            embed, blocks, _ = self.stage(i)
            embed.manipulate_width(meta["width"])
            for block in blocks:   # every block, skipped ones included
                block.manipulate(meta["width"], hidden_width(meta["mlp_ratio"], meta["width"]))

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        return {"body": {"depth": list(self.depths), "width": list(self.embed_dims),
                         "mlp_ratio": list(self.mlp_ratios)}}

    def active_blocks(self, i):
        blocks = self.stage(i)[1]
        return [blocks[j] for j in range(min(self.body_state["depth"][i], len(blocks)))]

    def prune_to_active(self, in_channels=3):
        """Physically cut the supernet to its current subnet, on whatever device it is: the blocks past each
        stage's depth go, every parameter keeps its active leading slice (tools/extract_subnet.py semantics;
        the forward pass of deploy mode starts with this)."""
        body, ci = self.body_state, in_channels
        for i in range(4):
            embed, blocks, norm = self.stage(i)
            c = body["width"][i]
            del blocks[body["depth"][i]:]
            if i == 0:
                convs_norms = ((embed.proj[0], embed.proj[1], c // 2), (embed.proj[3], embed.proj[4], c))
            else:
                convs_norms = ((embed.proj, embed.norm, c),)
            for conv, bn, co in convs_norms:
                conv._deploy_slice(ci)
                bn._deploy_slice(co)
                ci = co
            for block in blocks:
                block.prune(c, hidden_width(body["mlp_ratio"][i], c))
            norm._deploy_slice(c)
        self.embed_dims, self.depths = list(body["width"]), list(body["depth"])
        self.mlp_ratios = list(body["mlp_ratio"])

    # ---- execution ----
    def forward_act(self, tape, x):
        if getattr(self, "_deploying", False):
            self.prune_to_active(x.t.shape[1] if x.nchw_image else x.C)
        outs = []
        for i in range(4):
            embed, blocks, norm = self.stage(i)
            x = embed.forward_act(tape, x)
            for block in self.active_blocks(i):
                x = block.forward_act(tape, x)
            x = norm.forward_act(tape, x)
            if i == 0:
                streams.side_checkpoint(tape)   # as the other backbones: later layers' gradients are ready first
            if i in self.out_indices:
                outs.append(x)
        return outs

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def _stage_modules(self, i):
        embed, _, norm = self.stage(i)
        return [embed, norm] + self.active_blocks(i)

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (stage 1)."""
        return [p for m in self._stage_modules(0) for p in m.parameters()]

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: everything but the blocks the depth
        states skip."""
        return [m for i in range(4) for m in self._stage_modules(i)]
