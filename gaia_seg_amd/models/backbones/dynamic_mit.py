"""DynamicMixVisionTransformer backbone: SegFormer's Mix Transformer (MiT, arXiv 2105.15203) as a supernet.

Constructor after mmseg's ``MixVisionTransformer`` / transformers' ``SegformerConfig``; parameter and module
names are those of the encoder of transformers' ``SegformerModel`` (``stages.{i}.patch_embeddings.proj``,
``stages.{i}.blocks.{j}.attention.q_proj``, ...), so a ``SegformerModel`` state dict loads with
``strict=True`` (linear weights are 2-D, DynamicLinear).  MiT-B1..B5 are one architecture that differs in
depth per stage; head counts of 1/2/5/8 at head dimension 64 are what the attention kernels are built for.
The supernet is elastic in depth, head count (stage width = 64 x heads) and feed-forward ratio per stage:
search-space key ``body`` = {"depth": [4], "num_heads": [4], "mlp_ratio": [4]}, leading slices of every
parameter, only the first depth[i] blocks of a stage run.  Metas are only read.

``forward`` returns logical NCHW feature maps and runs the whole backbone as ONE autograd node over
hand-written HIP kernels, NHWC throughout: the stage map [B, H, W, D] IS the token matrix (no cls token, no
position embedding, no permutes).  A block computes

    x = x + o_proj(attn_kv(q_proj(LN(x)), k_proj(r), v_proj(r))),  r = LN(conv_{sr x sr, stride sr}(LN(x)))
    x = x + fc2(GELU(dwconv3x3(fc1(LN(x)))))                        (r = LN(x) where sr == 1)

with the overlapping patch embeddings (7x7 s4 p3 on the image, 3x3 s2 p1), the reduction convs and every
linear on gs_conv2d_*, the depthwise 3x3 on gs_dwconv2d_*, LayerNorm and GELU on csrc/convnext_ops.hip and
the attention -- all tokens of the stage against the tokens of the reduced map -- on gs_attention_kv_*
(csrc/attention_common.h).  K and V are written into the two column slices of one buffer.

Inputs must be multiples of 32 in both directions (every reduction conv then tiles its map exactly);
nothing depends on an ``img_size``, so whole-image and sliding-window evaluation both work.

Refused: ``drop_path_rate``, ``drop_rate``, ``attn_drop_rate > 0`` (stochastic depth and dropouts are not
implemented), and fp16 attention (``fp16 = dict(attention=True)``: gs_attention_kv_* has no fp16-operand
form).  Out of scope: MiT-B0 (head dimension 32), checkpoint key converters.
"""
import math

import torch.nn as nn

from ...core.bricks import DynamicConv2d, DynamicLayerNorm, DynamicLinear, GELU
from ...core.dynamic import DynamicMixin, unzip_meta
from ...hip import ops, streams
from ...hip.runtime import Act, tape_function
from ..builder import BACKBONES

HEAD_DIM = 64


def _refuse_positive(**kwargs):
    for key, value in kwargs.items():
        if value and value > 0:
            raise NotImplementedError("%s > 0 is not implemented (set %s=0)" % (key, key))


def hidden_width(mlp_ratio, width):
    """hidden width of the Mix-FFN (SegformerMixFFN: int(hidden_size * mlp_ratio))"""
    return int(mlp_ratio * width)


class MitPatchEmbeddings(nn.Module):
    """overlapping patch embedding: a strided conv with padding patch // 2, then LayerNorm"""

    def __init__(self, patch_size, stride, in_channels, width, eps):
        super().__init__()
        self.proj = DynamicConv2d(in_channels, width, patch_size, stride=stride, padding=patch_size // 2)
        self.layer_norm = DynamicLayerNorm(width, eps=eps)

    def forward_act(self, tape, x):
        return self.layer_norm.forward_act(tape, self.proj.forward_act(tape, x))


class MitSequenceReduction(nn.Module):
    """the map the keys and values come from: a sr x sr conv of stride sr, then LayerNorm"""

    def __init__(self, width, sr_ratio, eps):
        super().__init__()
        self.sequence_reduction = DynamicConv2d(width, width, sr_ratio, stride=sr_ratio)
        self.layer_norm = DynamicLayerNorm(width, eps=eps)

    def forward_act(self, tape, x):
        return self.layer_norm.forward_act(tape, self.sequence_reduction.forward_act(tape, x))


class MitAttention(nn.Module):
    """o_proj(softmax(scale * Q K^T) V): queries from every pixel, keys and values from the reduced map"""

    def __init__(self, width, num_heads, sr_ratio, eps):
        super().__init__()
        self.max_heads = self.num_heads = num_heads
        self.sr_ratio = sr_ratio
        self.scale = HEAD_DIM ** -0.5
        self.q_proj = DynamicLinear(width, width)
        self.k_proj = DynamicLinear(width, width)
        self.v_proj = DynamicLinear(width, width)
        self.o_proj = DynamicLinear(width, width)
        if sr_ratio > 1:
            self.sequence_reduction = MitSequenceReduction(width, sr_ratio, eps)

    def manipulate_num_heads(self, heads):
        self.num_heads = heads
        convs = [self.q_proj, self.k_proj, self.v_proj, self.o_proj]
        if self.sr_ratio > 1:
            convs.append(self.sequence_reduction.sequence_reduction)
        for conv in convs:
            conv.manipulate_width(heads * HEAD_DIM)

    def forward_act(self, tape, y):
        width = self.num_heads * HEAD_DIM
        r = self.sequence_reduction.forward_act(tape, y) if self.sr_ratio > 1 else y
        q = self.q_proj.forward_act(tape, y)
        kv = Act.empty(r.N, r.H, r.W, 2 * width, r.t.device)
        k, v = kv.slice(0, width), kv.slice(width, 2 * width)
        self.k_proj.forward_act(tape, r, out=k)
        self.v_proj.forward_act(tape, r, out=v)
        out = ops.attention_kv(tape, q, k, v, self.num_heads, self.scale)
        return self.o_proj.forward_act(tape, out)


class MitDWConv(nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.dwconv = DynamicConv2d(hidden, hidden, 3, padding=1, groups=hidden)


class MitMixFFN(nn.Module):
    """fc2(GELU(dwconv3x3(fc1(x))))"""

    def __init__(self, width, hidden):
        super().__init__()
        self.fc1 = DynamicLinear(width, hidden)
        self.dwconv = MitDWConv(hidden)
        self.act = GELU()
        self.fc2 = DynamicLinear(hidden, width)

    def manipulate(self, width, hidden):
        self.fc1.manipulate_width(hidden)
        self.dwconv.dwconv.manipulate_width(hidden)
        self.fc2.manipulate_width(width)

    def forward_act(self, tape, x):
        z = self.fc1.forward_act(tape, x)
        z = self.dwconv.dwconv.forward_act(tape, z)
        z = self.act.forward_act(tape, z)
        return self.fc2.forward_act(tape, z)


class MitBlock(nn.Module):
    def __init__(self, width, num_heads, sr_ratio, hidden, eps):
        super().__init__()
        self.layernorm_before = DynamicLayerNorm(width, eps=eps)
        self.attention = MitAttention(width, num_heads, sr_ratio, eps)
        self.layernorm_after = DynamicLayerNorm(width, eps=eps)
        self.mlp = MitMixFFN(width, hidden)

    def forward_act(self, tape, x):
        a = self.attention.forward_act(tape, self.layernorm_before.forward_act(tape, x))
        x = ops.layer_scale_add(tape, x, a, None)
        z = self.mlp.forward_act(tape, self.layernorm_after.forward_act(tape, x))
        return ops.layer_scale_add(tape, x, z, None)


class MitStage(nn.Module, DynamicMixin):
    """patch embedding, ``depth`` blocks at their maximum size (only the first ``depth_state`` run), LayerNorm"""
    search_space = {"depth", "num_heads", "mlp_ratio"}

    def __init__(self, in_channels, num_heads, depth, patch_size, stride, sr_ratio, mlp_ratio, eps):
        super().__init__()
        width = HEAD_DIM * num_heads
        self.max_heads, self.max_ratio = num_heads, mlp_ratio
        self.patch_embeddings = MitPatchEmbeddings(patch_size, stride, in_channels, width, eps)
        self.blocks = nn.ModuleList([MitBlock(width, num_heads, sr_ratio, hidden_width(mlp_ratio, width), eps)
                                     for _ in range(depth)])
        self.layer_norm = DynamicLayerNorm(width, eps=eps)
        self.init_state(depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio)

    def manipulate_depth(self, depth):
        if not 1 <= depth <= len(self.blocks):
            raise ValueError("depth %s out of range (1..%d)" % (depth, len(self.blocks)))
        self.depth_state = depth

    def manipulate_num_heads(self, heads):
        if not (isinstance(heads, int) and 1 <= heads <= self.max_heads):
            raise ValueError("num_heads %s out of range (1..%d)" % (heads, self.max_heads))
        self.num_heads_state = heads
        self._apply_widths()

    def manipulate_mlp_ratio(self, ratio):
        if not 0 < ratio <= self.max_ratio:
            raise ValueError("mlp_ratio %s out of range (0..%s]" % (ratio, self.max_ratio))
        self.mlp_ratio_state = ratio
        self._apply_widths()

    def _apply_widths(self):
        width = HEAD_DIM * self.num_heads_state
        hidden = hidden_width(self.mlp_ratio_state, width)
        if hidden % 4 or hidden <= 0:
            raise ValueError("mlp_ratio %s: the hidden width int(%s * %d) = %d is no multiple of 4"
                             % (self.mlp_ratio_state, self.mlp_ratio_state, width, hidden))
        self.patch_embeddings.proj.manipulate_width(width)
        for block in self.blocks:   # every block, skipped ones included
            block.attention.manipulate_num_heads(self.num_heads_state)
            block.mlp.manipulate(width, hidden)

    def active_blocks(self):
        return [self.blocks[i] for i in range(self.depth_state)]

    def active_modules(self):
        return [self.patch_embeddings, self.layer_norm] + self.active_blocks()

    def forward_act(self, tape, x):
        if getattr(self, "_deploying", False):
            del self.blocks[self.depth_state:]
        x = self.patch_embeddings.forward_act(tape, x)
        for block in self.active_blocks():
            x = block.forward_act(tape, x)
        return self.layer_norm.forward_act(tape, x)


@BACKBONES.register_module()
class DynamicMixVisionTransformer(nn.Module, DynamicMixin):
    """Mix Transformer encoder with, per stage, elastic depth, head count (width = 64 x heads) and
    feed-forward ratio."""
    search_space = {"body"}

    def __init__(self, in_channels=3, num_stages=4, num_layers=(2, 2, 2, 2), num_heads=(1, 2, 5, 8),
                 patch_sizes=(7, 3, 3, 3), strides=(4, 2, 2, 2), sr_ratios=(8, 4, 2, 1), mlp_ratio=4,
                 out_indices=(0, 1, 2, 3), drop_path_rate=0., drop_rate=0., attn_drop_rate=0.,
                 norm_cfg=dict(type="LN", eps=1e-6), pretrained=None):
        super().__init__()
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        _refuse_positive(drop_path_rate=drop_path_rate, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate)
        if norm_cfg.get("type") not in ("LN", "DynLN"):
            raise NotImplementedError("norm_cfg: LayerNorm (type 'LN') is the only norm of the Mix Transformer")
        eps = norm_cfg.get("eps", 1e-6)
        if num_stages != 4:
            raise NotImplementedError("num_stages: the Mix Transformer has four stages")
        ratios = list(mlp_ratio) if isinstance(mlp_ratio, (list, tuple)) else [mlp_ratio] * 4
        for key, value in (("num_layers", num_layers), ("num_heads", num_heads), ("patch_sizes", patch_sizes),
                           ("strides", strides), ("sr_ratios", sr_ratios), ("mlp_ratio", ratios)):
            if len(value) != 4:
                raise ValueError("%s needs four entries, one per stage (got %s)" % (key, (value,)))
        if tuple(strides) != (4, 2, 2, 2) or any(sr * s > 32 or 32 % (sr * s) for sr, s in
                                                 zip(sr_ratios, (4, 8, 16, 32))):
            raise NotImplementedError("strides %s / sr_ratios %s: strides 4, 2, 2, 2 and reduction ratios that "
                                      "tile a 32-pixel cell of the input" % ((strides,), (sr_ratios,)))
        self.num_layers, self.num_heads, self.mlp_ratios = list(num_layers), list(num_heads), ratios
        self.sr_ratios, self.out_indices = list(sr_ratios), list(out_indices)
        self.init_state(body=self.full_arch_meta()["body"])
        stages, ci = [], in_channels
        for i in range(4):
            stages.append(MitStage(ci, num_heads[i], num_layers[i], patch_sizes[i], strides[i], sr_ratios[i],
                                   ratios[i], eps))
            ci = HEAD_DIM * num_heads[i]
        self.stages = nn.ModuleList(stages)
        self.init_weights(pretrained)

    # gs_attention_kv_* has no fp16-operand form: wrap_fp16_model(attention=True) is refused here
    @property
    def fp16_attention(self):
        return False

    @fp16_attention.setter
    def fp16_attention(self, flag):
        if flag:
            raise NotImplementedError("fp16.attention: DynamicMixVisionTransformer's attention "
                                      "(gs_attention_kv_*) has no fp16-operand form (set fp16.attention=False)")

    def init_weights(self, pretrained=None):
        """mmseg's MixVisionTransformer init: truncated normal (std 0.02) linears, fan-out normal convs, zero
        biases, unit LayerNorms; then the checkpoint, if a path is given."""
        for m in self.modules():
            if isinstance(m, DynamicLinear):
                nn.init.trunc_normal_(m.weight, std=.02)
            elif isinstance(m, DynamicConv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0, math.sqrt(2.0 / fan_out))
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)
            if isinstance(m, DynamicConv2d) and m.bias is not None:
                nn.init.constant_(m.bias, 0)
        if isinstance(pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)

    # ---- arch manipulation ----
    def manipulate_body(self, arch_meta):
        """{'depth': [d1..d4], 'num_heads': [h1..h4], 'mlp_ratio': [r1..r4]}: one entry per stage; the next
        stage's patch embedding follows the width of the stage that feeds it.  The meta is only read."""
        for key in ("depth", "num_heads", "mlp_ratio"):
            if key not in arch_meta or len(arch_meta[key]) != 4:
                raise ValueError("body.%s: four entries, one per stage (got %s)" % (key, arch_meta.get(key)))
        self.body_state = arch_meta
        for stage, meta in zip(self.stages, unzip_meta({k: arch_meta[k] for k in ("depth", "num_heads",
                                                                                 "mlp_ratio")})):
            stage.manipulate_arch(meta)

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        return {"body": {"depth": list(self.num_layers), "num_heads": list(self.num_heads),
                         "mlp_ratio": list(self.mlp_ratios)}}

    # ---- execution ----
    def forward_act(self, tape, x):
        h, w = (x.t.shape[2], x.t.shape[3]) if x.nchw_image else (x.H, x.W)
        if h % 32 or w % 32:
            raise ValueError("DynamicMixVisionTransformer: input size %d x %d is no multiple of 32 in both "
                             "directions (the reduction convs must tile their maps)" % (h, w))
        outs = []
        for i, stage in enumerate(self.stages):
            x = stage.forward_act(tape, x)
            if i == 0:
                streams.side_checkpoint(tape)   # as the other backbones: later layers' gradients are ready first
            if i in self.out_indices:
                outs.append(x)
        return outs

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (stage 1)."""
        return [p for m in self.stages[0].active_modules() for p in m.parameters()]

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: everything but the blocks the depth
        states skip."""
        return [m for stage in self.stages for m in stage.active_modules()]
