"""DynamicSwinTransformer backbone: the Swin Transformer (arXiv 2103.14030) as a supernet.

Constructor after mmseg's ``SwinTransformer`` / transformers' ``SwinConfig``; parameter and module names are
those of transformers' ``SwinBackbone`` with all four ``out_features`` (``swin.embeddings.patch_embeddings.
projection``, ``swin.encoder.layers.{i}.blocks.{j}.attention.q_proj``, ``swin.encoder.layers.{i}.downsample.
{reduction, norm}``, ``hidden_states_norms.stage{k}``, ...), so its state dict loads with ``strict=True``.
``swin.layernorm`` is kept as a parameter and never read.  Swin-T / S / B are one architecture that differs in
the depth of stage 3 and in the head count at head dimension 32: search-space key ``body`` = {"depth": [4],
"num_heads": [4], "mlp_ratio": [4]}, stage width = 32 x heads independently per stage, leading slices of every
parameter, only the first depth[i] blocks of a stage run.  The patch merging slices group-wise: its norm and
its reduction keep transformers' [4 Cmax] order in the state dict, and a subnet of width C reads the leading C
channels of each of the four 2x2 phases.  Metas are only read.

Semantics are ``SwinBackbone``'s (``always_partition``): the window stays ``window_size`` at every resolution,
block j shifts by 0 (j even) or window_size // 2 (j odd), features are the stage outputs before downsampling
through ``hidden_states_norms``.  One autograd node, NHWC throughout, the stage map IS the token matrix:

    y = LN(x), zero-padded to a multiple of the window (ops.map_pad; no launch when it already is one)
    x = x + o_proj(crop(window_attention(q_proj(y), k_proj(y), v_proj(y), table)))
    x = x + fc2(GELU(fc1(LN(x))))
    merge: reduction_{2x2 stride 2, no bias}(cell_layernorm(x))

(o_proj acts per token, so cropping before it equals transformers' cropping after it.)  The attention runs on
gs_window_attention_* (csrc/window_attention.hip) in fp32 in every precision mode.

Inputs must be multiples of 32 in both directions, so no merge meets an odd map.  Refused: ``drop_path_rate``,
``drop_rate``, ``attn_drop_rate > 0``, ``use_abs_pos_embed``, a ``window_size`` outside 2..8, a checkpoint
table of another window size (no interpolation on load), ``fp16 = dict(attention=True)``.
"""
import torch
import torch.nn as nn

from ...core.bricks import DynamicConv2d, DynamicLayerNorm, DynamicLinear, GELU
from ...core.dynamic import DynamicMixin, unzip_meta
from ...hip import ops, streams
from ...hip.runtime import Act, tape_function
from ..builder import BACKBONES

HEAD_DIM = 32


def _refuse_positive(**kwargs):
    for key, value in kwargs.items():
        if value and value > 0:
            raise NotImplementedError("%s > 0 is not implemented (set %s=0)" % (key, key))


def hidden_width(mlp_ratio, width):
    return int(mlp_ratio * width)


class SwinRelativePositionBias(nn.Module):
    """the learned table [(2 ws - 1)^2, heads]; the kernel gathers from it"""

    def __init__(self, num_heads, window_size):
        super().__init__()
        self.window_size = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        t = state_dict.get(prefix + "relative_position_bias_table")
        if t is not None and t.shape[0] != self.relative_position_bias_table.shape[0]:
            raise NotImplementedError("%srelative_position_bias_table has %d rows, window_size %d needs %d: a "
                                      "checkpoint of another window size is not interpolated on load"
                                      % (prefix, t.shape[0], self.window_size,
                                         self.relative_position_bias_table.shape[0]))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class SwinAttention(nn.Module):
    def __init__(self, width, num_heads, window_size, qkv_bias):
        super().__init__()
        self.num_heads, self.window_size = num_heads, window_size
        self.scale = HEAD_DIM ** -0.5
        self.q_proj = DynamicLinear(width, width, bias=qkv_bias)
        self.k_proj = DynamicLinear(width, width, bias=qkv_bias)
        self.v_proj = DynamicLinear(width, width, bias=qkv_bias)
        self.o_proj = DynamicLinear(width, width)
        self.relative_position_bias = SwinRelativePositionBias(num_heads, window_size)

    def manipulate_num_heads(self, heads):
        self.num_heads = heads
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.o_proj):
            lin.manipulate_width(heads * HEAD_DIM)

    def forward_act(self, tape, y, shift):
        ws, width = self.window_size, self.num_heads * HEAD_DIM
        h, w = y.H, y.W
        hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
        padded = (hp, wp) != (h, w)
        if padded:
            y = ops.map_pad(tape, y, hp, wp)
        qkv = Act.empty(y.N, hp, wp, 3 * width, y.t.device)
        q, k, v = qkv.slice(0, width), qkv.slice(width, 2 * width), qkv.slice(2 * width, 3 * width)
        self.q_proj.forward_act(tape, y, out=q)
        self.k_proj.forward_act(tape, y, out=k)
        self.v_proj.forward_act(tape, y, out=v)
        out = ops.window_attention(tape, q, k, v, self.relative_position_bias.relative_position_bias_table,
                                   self.num_heads, ws, shift, self.scale)
        if padded:
            out = ops.map_crop(tape, out, h, w)
        return self.o_proj.forward_act(tape, out)


class SwinMLP(nn.Module):
    def __init__(self, width, hidden):
        super().__init__()
        self.fc1 = DynamicLinear(width, hidden)
        self.act = GELU()
        self.fc2 = DynamicLinear(hidden, width)

    def manipulate(self, width, hidden):
        self.fc1.manipulate_width(hidden)
        self.fc2.manipulate_width(width)

    def forward_act(self, tape, x):
        return self.fc2.forward_act(tape, self.act.forward_act(tape, self.fc1.forward_act(tape, x)))


class SwinBlock(nn.Module):
    def __init__(self, width, num_heads, window_size, shift, hidden, qkv_bias, eps):
        super().__init__()
        self.shift = shift
        self.layernorm_before = DynamicLayerNorm(width, eps=eps)
        self.attention = SwinAttention(width, num_heads, window_size, qkv_bias)
        self.layernorm_after = DynamicLayerNorm(width, eps=eps)
        self.mlp = SwinMLP(width, hidden)

    def forward_act(self, tape, x):
        a = self.attention.forward_act(tape, self.layernorm_before.forward_act(tape, x), self.shift)
        x = ops.layer_scale_add(tape, x, a, None)
        z = self.mlp.forward_act(tape, self.layernorm_after.forward_act(tape, x))
        return ops.layer_scale_add(tape, x, z, None)


class SwinMergeReduction(DynamicConv2d):
    """transformers' ``reduction = Linear(4 C, C_next, bias=False)`` on the concatenated 2x2 phases, held as the
    2x2 stride-2 convolution it is.  The state dict presents the 2-D weight [C_next, 4 Cmax] in transformers'
    order (column (2 col + row) * Cmax + c); the conv's input slice -- the leading C channels of every tap --
    is the group-wise slice of that matrix."""

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, out_channels, 2, stride=2, bias=False)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        w = destination[prefix + "weight"]                       # [o, c, row, col]
        destination[prefix + "weight"] = w.permute(0, 3, 2, 1).reshape(w.shape[0], -1)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + "weight")
        if w is not None and w.dim() == 2:
            state_dict = dict(state_dict)
            state_dict[prefix + "weight"] = w.reshape(w.shape[0], 2, 2, -1).permute(0, 3, 2, 1).clone()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class SwinMergeNorm(nn.LayerNorm):
    """LayerNorm(4 Cmax) of the concatenated phases, run on the map itself (ops.cell_layernorm)"""

    def forward_act(self, tape, x):
        return ops.cell_layernorm(tape, x, self.weight, self.bias, self.eps)


class SwinPatchMerging(nn.Module):
    def __init__(self, width, next_width, eps):
        super().__init__()
        self.reduction = SwinMergeReduction(width, next_width)
        self.norm = SwinMergeNorm(4 * width, eps=eps)

    def forward_act(self, tape, x):
        return self.reduction.forward_act(tape, self.norm.forward_act(tape, x))


class SwinStage(nn.Module, DynamicMixin):
    """``depth`` blocks at their maximum size (only the first ``depth_state`` run), then the patch merging"""
    search_space = {"depth", "num_heads", "mlp_ratio"}

    def __init__(self, num_heads, next_heads, depth, window_size, mlp_ratio, qkv_bias, eps):
        super().__init__()
        width = HEAD_DIM * num_heads
        self.max_heads, self.max_ratio = num_heads, mlp_ratio
        self.blocks = nn.ModuleList([
            SwinBlock(width, num_heads, window_size, 0 if j % 2 == 0 else window_size // 2,
                      hidden_width(mlp_ratio, width), qkv_bias, eps) for j in range(depth)])
        if next_heads is not None:
            self.downsample = SwinPatchMerging(width, HEAD_DIM * next_heads, eps)
        else:
            self.downsample = None
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
        for block in self.blocks:   # every block, skipped ones included
            block.attention.manipulate_num_heads(self.num_heads_state)
            block.mlp.manipulate(width, hidden)

    def active_blocks(self):
        return [self.blocks[i] for i in range(self.depth_state)]

    def forward_blocks(self, tape, x):
        if getattr(self, "_deploying", False):
            del self.blocks[self.depth_state:]
        for block in self.active_blocks():
            x = block.forward_act(tape, x)
        return x


class SwinPatchEmbeddings(nn.Module):
    def __init__(self, in_channels, width, patch_size):
        super().__init__()
        self.projection = DynamicConv2d(in_channels, width, patch_size, stride=patch_size)


class SwinEmbeddings(nn.Module):
    def __init__(self, in_channels, width, patch_size, eps):
        super().__init__()
        self.patch_embeddings = SwinPatchEmbeddings(in_channels, width, patch_size)
        self.norm = DynamicLayerNorm(width, eps=eps)

    def forward_act(self, tape, x):
        return self.norm.forward_act(tape, self.patch_embeddings.projection.forward_act(tape, x))


class SwinEncoder(nn.Module):
    def __init__(self, stages):
        super().__init__()
        self.layers = nn.ModuleList(stages)


class SwinBody(nn.Module):
    def __init__(self, embeddings, stages, last_width, eps):
        super().__init__()
        self.embeddings = embeddings
        self.encoder = SwinEncoder(stages)
        self.layernorm = DynamicLayerNorm(last_width, eps=eps)   # SwinModel's final norm: never read here


@BACKBONES.register_module()
class DynamicSwinTransformer(nn.Module, DynamicMixin):
    """Swin encoder with, per stage, elastic depth, head count (width = 32 x heads) and MLP ratio."""
    search_space = {"body"}

    def __init__(self, in_channels=3, patch_size=4, window_size=7, mlp_ratio=4, depths=(2, 2, 18, 2),
                 num_heads=(4, 8, 16, 32), out_indices=(0, 1, 2, 3), qkv_bias=True, drop_path_rate=0.,
                 drop_rate=0., attn_drop_rate=0., use_abs_pos_embed=False, norm_cfg=dict(type="LN", eps=1e-5),
                 pretrained=None):
        super().__init__()
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        _refuse_positive(drop_path_rate=drop_path_rate, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate)
        if use_abs_pos_embed:
            raise NotImplementedError("use_abs_pos_embed=True is not implemented (set use_abs_pos_embed=False)")
        if not (isinstance(window_size, int) and 2 <= window_size <= 8):
            raise NotImplementedError("window_size %s: gs_window_attention_* handles window_size 2..8"
                                      % (window_size,))
        if patch_size != 4:
            raise NotImplementedError("patch_size %s: the 4x4 stride-4 patch embedding is the only one" % patch_size)
        if norm_cfg.get("type") not in ("LN", "DynLN"):
            raise NotImplementedError("norm_cfg: LayerNorm (type 'LN') is the only norm of the Swin Transformer")
        eps = norm_cfg.get("eps", 1e-5)
        ratios = list(mlp_ratio) if isinstance(mlp_ratio, (list, tuple)) else [mlp_ratio] * 4
        for key, value in (("depths", depths), ("num_heads", num_heads), ("mlp_ratio", ratios)):
            if len(value) != 4:
                raise ValueError("%s needs four entries, one per stage (got %s)" % (key, (value,)))
        self.depths, self.num_heads, self.mlp_ratios = list(depths), list(num_heads), ratios
        self.window_size, self.out_indices = window_size, list(out_indices)
        self.init_state(body=self.full_arch_meta()["body"])
        stages = [SwinStage(num_heads[i], num_heads[i + 1] if i < 3 else None, depths[i], window_size, ratios[i],
                            qkv_bias, eps) for i in range(4)]
        self.swin = SwinBody(SwinEmbeddings(in_channels, HEAD_DIM * num_heads[0], patch_size, eps), stages,
                             HEAD_DIM * num_heads[3], eps)
        self.hidden_states_norms = nn.ModuleDict({"stage%d" % (i + 1): DynamicLayerNorm(HEAD_DIM * num_heads[i], eps=eps)
                                                  for i in range(4)})
        self.init_weights(pretrained)

    @property
    def stages(self):
        return self.swin.encoder.layers

    # gs_window_attention_* is fp32 only: wrap_fp16_model(attention=True) is refused here
    @property
    def fp16_attention(self):
        return False

    @fp16_attention.setter
    def fp16_attention(self, flag):
        if flag:
            raise NotImplementedError("fp16.attention: DynamicSwinTransformer's attention "
                                      "(gs_window_attention_*) has no fp16-operand form (set fp16.attention=False)")

    def init_weights(self, pretrained=None):
        """truncated normal (std 0.02) linears and tables, zero biases, unit LayerNorms; then the checkpoint"""
        for m in self.modules():
            if isinstance(m, DynamicConv2d):
                nn.init.trunc_normal_(m.weight, std=.02)
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
        """{'depth': [d1..d4], 'num_heads': [h1..h4], 'mlp_ratio': [r1..r4]}: one entry per stage; a merge's
        reduction follows the width of the stage it feeds.  The meta is only read."""
        for key in ("depth", "num_heads", "mlp_ratio"):
            if key not in arch_meta or len(arch_meta[key]) != 4:
                raise ValueError("body.%s: four entries, one per stage (got %s)" % (key, arch_meta.get(key)))
        self.body_state = arch_meta
        metas = unzip_meta({k: arch_meta[k] for k in ("depth", "num_heads", "mlp_ratio")})
        for stage, meta in zip(self.stages, metas):
            stage.manipulate_arch(meta)
        heads = [stage.num_heads_state for stage in self.stages]
        self.swin.embeddings.patch_embeddings.projection.manipulate_width(HEAD_DIM * heads[0])
        for i in range(3):
            self.stages[i].downsample.reduction.manipulate_width(HEAD_DIM * heads[i + 1])

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        return {"body": {"depth": list(self.depths), "num_heads": list(self.num_heads),
                         "mlp_ratio": list(self.mlp_ratios)}}

    # ---- execution ----
    def forward_act(self, tape, x):
        h, w = (x.t.shape[2], x.t.shape[3]) if x.nchw_image else (x.H, x.W)
        if h % 32 or w % 32:
            raise ValueError("DynamicSwinTransformer: input size %d x %d is no multiple of 32 in both directions "
                             "(a patch merging must not meet an odd map)" % (h, w))
        outs = []
        x = self.swin.embeddings.forward_act(tape, x)
        for i, stage in enumerate(self.stages):
            x = stage.forward_blocks(tape, x)
            if i == 0:
                streams.side_checkpoint(tape)   # as the other backbones: later layers' gradients are ready first
            if i in self.out_indices:
                outs.append(self.hidden_states_norms["stage%d" % (i + 1)].forward_act(tape, x))
            if stage.downsample is not None:
                x = stage.downsample.forward_act(tape, x)
        return outs

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (embeddings and stage 1)."""
        mods = [self.swin.embeddings] + self.stages[0].active_blocks()
        return [p for m in mods for p in m.parameters()]

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: everything but the blocks the depth states
        skip, ``swin.layernorm`` (never read) and the output norms of stages that are not returned."""
        mods = [self.swin.embeddings]
        for i, stage in enumerate(self.stages):
            mods += stage.active_blocks()
            if stage.downsample is not None:
                mods.append(stage.downsample)
            if i in self.out_indices:
                mods.append(self.hidden_states_norms["stage%d" % (i + 1)])
        return mods
