"""BEiT backbone — host-side mirror of gaiaseg/models/backbones/beit.py, forward only.

The reference's DynamicDistiller was written for a BEiT teacher; this module exists so that the public
BEiT UPerNet checkpoints load and run as that frozen teacher.  Same registered name, constructor
signature and defaults, attribute / parameter / buffer names and shapes (both ``patch_size`` branches of
``fpn1..4``) and the same initialisation.  ``forward`` returns the four pyramid maps as logical NCHW
tensors and runs on hand-written HIP kernels only: the patch embedding and every linear on gs_conv2d_*
(``qkv`` is ONE launch D -> 3 D with the bias cat(q_bias, 0, v_bias); Q, K, V are column slices of its
output), LayerNorm / GELU / ``x + gamma * branch`` on csrc/convnext_ops.hip, the token assembly on
gs_vit_tokens_*, attention on gs_attention_relpos_forward (the relative-position bias is gathered from the
table inside the kernel; no N x N bias is ever built) or gs_attention_forward where a block has no bias,
``ConvTranspose2d(2, 2)`` on gs_deconv2x2_forward, SyncBN in eval on the BatchNorm kernels with running
statistics and the max-pools on gs_maxpool_forward.

Forward only: the module is a frozen teacher and runs in eval mode.  Dropout and drop-path rates are
accepted and inert.  Calling it so that a gradient would be needed -- grad mode on and a parameter (or the
input) that requires grad -- raises NotImplementedError: there is no attention backward with a bias
gradient and no deconvolution backward.

Departures from the reference, on purpose:

* ``relative_position_index`` ([N, N] int64, 34 MB per block at a 32 x 64 window) is not held as a buffer:
  the kernel computes the index.  ``state_dict()`` still writes it (built on the host when saving) and a
  checkpoint that carries it loads; the values are ignored, as the reference pops them.
* ``init_weights(None)`` keeps the constructor's initialisation (the reference re-draws every linear there
  and thereby undoes ``fix_init_weight``).
* ``relative_position_bias_table`` / ``pos_embed`` of another size than the model's are refused on load;
  the reference interpolates them (``deal_with_position_embedding``), which is not implemented.

Refused by name: ``hybrid_backbone``, ``norm_layer``, a ``patch_size`` other than 8 / 16, a head dimension
other than 64, an ``out_indices`` that does not name exactly four blocks and an input whose size is not
``img_size`` (evaluation slides a window of that size).  ``use_checkpoint`` is accepted and ignored.
"""
import math

import torch
import torch.nn as nn

from ...core.bricks import GELU, DynamicConv2d, DynamicLayerNorm, DynamicLinear, build_norm_layer
from ...hip import lib as _lib
from ...hip import ops
from ...hip.runtime import tape_function
from ..builder import BACKBONES

HEAD_DIM = 64
FORWARD_ONLY = ("BEiT: forward only (frozen teacher); there is no backward for the biased attention and the "
                "deconvolution -- call it under torch.no_grad() or freeze its parameters")


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def relative_position_index(window_size):
    """BEiT's [N, N] index into a relative_position_bias_table for a (Wh, Ww) window, N = Wh * Ww + 1 with
    the cls token first: (iy - jy + Wh - 1) * (2 Ww - 1) + (ix - jx + Ww - 1) between patches, and rows R,
    R + 1, R + 2 (R = (2 Wh - 1)(2 Ww - 1)) for cls -> patch, patch -> cls, cls -> cls.  The host-side
    statement of what gs_attention_relpos_forward computes per score."""
    wh, ww = window_size
    r = (2 * wh - 1) * (2 * ww - 1)
    ys, xs = torch.arange(wh).repeat_interleave(ww), torch.arange(ww).repeat(wh)
    idx = torch.empty((wh * ww + 1, wh * ww + 1), dtype=torch.int64)
    idx[1:, 1:] = (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)
    idx[0, :] = r
    idx[:, 0] = r + 1
    idx[0, 0] = r + 2
    return idx


class _RelPosTable(nn.Module):
    """A relative_position_bias_table parameter and the state-dict face of its index (module docstring)."""

    def _init_table(self, window_size, num_heads):
        self.window_size = tuple(window_size)
        self.num_relative_distance = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) + 3
        if self.num_relative_distance > _lib.ATTENTION_RELPOS_MAX_ROWS:
            raise ValueError("img_size: a %d x %d patch window needs %d relative positions, the attention "
                             "kernel holds at most %d" % (window_size[0], window_size[1],
                                                          self.num_relative_distance,
                                                          _lib.ATTENTION_RELPOS_MAX_ROWS))
        self.relative_position_bias_table = nn.Parameter(torch.zeros(self.num_relative_distance, num_heads))

    @property
    def relative_position_index(self):
        return relative_position_index(self.window_size) if self.window_size else None

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.window_size:
            destination[prefix + "relative_position_index"] = self.relative_position_index

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.pop(prefix + "relative_position_index", None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class RelativePositionBias(_RelPosTable):
    """The bias table shared by all blocks (``use_shared_rel_pos_bias``)."""

    def __init__(self, window_size, num_heads):
        super().__init__()
        self._init_table(window_size, num_heads)


class Attention(_RelPosTable):
    fp16_attention = False   # set through BEiT.fp16_attention

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.,
                 window_size=None, attn_head_dim=None):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads if attn_head_dim is None else attn_head_dim
        if head_dim != HEAD_DIM:
            raise NotImplementedError("attn_head_dim / embed_dim // num_heads: the attention kernels have a "
                                      "head dimension of %d, got %d" % (HEAD_DIM, head_dim))
        all_head_dim = head_dim * num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = DynamicLinear(dim, all_head_dim * 3, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(all_head_dim))
            self.v_bias = nn.Parameter(torch.zeros(all_head_dim))
        else:
            self.q_bias = self.v_bias = None
        if window_size:
            self._init_table(window_size, num_heads)
        else:
            self.window_size = None
            self.relative_position_bias_table = None
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = DynamicLinear(all_head_dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _qkv_bias(self):
        """cat(q_bias, 0, v_bias), remade when either parameter has been written to or moved"""
        if self.q_bias is None:
            return None
        key = (self.q_bias._version, self.v_bias._version, self.q_bias.data_ptr(), self.v_bias.data_ptr())
        cached = self.__dict__.get("_qkv_bias_cache")
        if cached is None or cached[0] != key:
            q, v = self.q_bias.detach(), self.v_bias.detach()
            cached = self.__dict__["_qkv_bias_cache"] = (key, torch.cat((q, torch.zeros_like(v), v)))
        return cached[1]

    def forward_act(self, tape, x, table, window):
        """``table``: this block's table plus the shared one (either may be missing), or None"""
        width = self.num_heads * HEAD_DIM
        self.qkv._check_layout()
        qkv = ops.conv2d(tape, x, self.qkv.weight, self._qkv_bias(), 3 * width)
        q, k, v = (qkv.slice(i * width, (i + 1) * width) for i in range(3))
        if table is None:
            out = ops.attention(tape, q, k, v, self.num_heads, self.scale, f16=self.fp16_attention)
        else:
            out = ops.attention_relpos(tape, q, k, v, self.num_heads, self.scale, table, window,
                                       f16=self.fp16_attention)
        return self.proj.forward_act(tape, out)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = DynamicLinear(in_features, hidden_features)
        self.act = GELU()
        self.fc2 = DynamicLinear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward_act(self, tape, x):
        return self.fc2.forward_act(tape, self.act.forward_act(tape, self.fc1.forward_act(tape, x)))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., init_values=None, window_size=None, attn_head_dim=None):
        super().__init__()
        self.norm1 = DynamicLayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                              attn_drop=attn_drop, proj_drop=drop, window_size=window_size,
                              attn_head_dim=attn_head_dim)
        self.drop_path = nn.Identity()   # stochastic depth is inert in eval mode
        self.norm2 = DynamicLayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), drop=drop)
        if init_values is not None:
            self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
            self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))
        else:
            self.gamma_1 = self.gamma_2 = None

    def forward_act(self, tape, x, table, window):
        branch = self.attn.forward_act(tape, self.norm1.forward_act(tape, x), table, window)
        x = ops.layer_scale_add(tape, x, branch, self.gamma_1)
        branch = self.mlp.forward_act(tape, self.norm2.forward_act(tape, x))
        return ops.layer_scale_add(tape, x, branch, self.gamma_2)


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        img_size, patch_size = _pair(img_size), _pair(patch_size)
        self.patch_shape = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.num_patches = self.patch_shape[0] * self.patch_shape[1]
        self.img_size, self.patch_size = img_size, patch_size
        self.proj = DynamicConv2d(in_chans, embed_dim, kernel_size=patch_size[0], stride=patch_size[0])

    def forward_act(self, tape, x):
        h, w = (x.t.shape[2], x.t.shape[3]) if x.nchw_image else (x.H, x.W)
        if (h, w) != self.img_size:
            raise ValueError("img_size: input image size (%d*%d) doesn't match model (%d*%d)"
                             % (h, w, self.img_size[0], self.img_size[1]))
        return self.proj.forward_act(tape, x)


class ConvTranspose2x2(nn.Module):
    """nn.ConvTranspose2d(in_channels, out_channels, kernel_size=2, stride=2): torch's parameter names,
    layout ([Cin, Cout, 2, 2]) and default initialisation, forward on gs_deconv2x2_forward."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, 2, 2))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(out_channels * 4)   # torch's fan_in of a transposed-conv weight
        nn.init.uniform_(self.bias, -bound, bound)

    def forward_act(self, tape, x):
        return ops.deconv2x2(tape, x, self.weight, self.bias)


class MaxPool(nn.Module):
    """nn.MaxPool2d(kernel_size=k, stride=k)"""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = self.stride = kernel_size

    def forward_act(self, tape, x):
        return ops.maxpool(tape, x, k=self.kernel_size, s=self.stride, p=0)


def _run(tape, module, x):
    """a pyramid branch: nn.Identity, one operator module, or an nn.Sequential of them"""
    if isinstance(module, nn.Identity):
        return x
    if isinstance(module, nn.Sequential):
        for m in module:
            x = _run(tape, m, x)
        return x
    return module.forward_act(tape, x)


@BACKBONES.register_module()
class BEiT(nn.Module):
    """Vision transformer with BEiT's relative-position bias and a four-level pyramid on top."""
    _fp16_attention = False

    @property
    def fp16_attention(self):
        """Opt-in, as ElasticTransformer.fp16_attention: inside an fp16 mode every attention runs on the
        fp16-operand kernels (the bias stays fp32)."""
        return self._fp16_attention

    @fp16_attention.setter
    def fp16_attention(self, flag):
        self._fp16_attention = bool(flag)
        for m in self.modules():
            if isinstance(m, Attention):
                m.fp16_attention = self._fp16_attention

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=80, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., hybrid_backbone=None, norm_layer=None, init_values=None,
                 use_checkpoint=False, use_abs_pos_emb=True, use_rel_pos_bias=False,
                 use_shared_rel_pos_bias=False, out_indices=[3, 5, 7, 11]):
        super().__init__()
        if hybrid_backbone is not None:
            raise NotImplementedError("hybrid_backbone: the CNN patch embedding (HybridEmbed) is not "
                                      "implemented")
        if norm_layer is not None:
            raise NotImplementedError("norm_layer: only the default LayerNorm(eps=1e-6) is implemented")
        if patch_size not in (8, 16):
            raise NotImplementedError("patch_size: the reference builds fpn1..4 for 8 and 16 only, got %r"
                                      % (patch_size,))
        out_indices = list(out_indices)
        if len(set(out_indices)) != 4 or len(out_indices) != 4 or any(not 0 <= i < depth for i in out_indices):
            raise ValueError("out_indices: fpn1..4 are applied by position, so exactly four blocks of 0..%d "
                             "must be named, got %s" % (depth - 1, out_indices))
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans,
                                      embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        window = self.patch_embed.patch_shape
        self.out_indices = out_indices
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        if use_abs_pos_emb:
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        else:
            self.pos_embed = None
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.rel_pos_bias = RelativePositionBias(window, num_heads) if use_shared_rel_pos_bias else None
        self.use_rel_pos_bias = use_rel_pos_bias
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, init_values=init_values,
                  window_size=window if use_rel_pos_bias else None)
            for _ in range(depth)])
        if self.pos_embed is not None:
            nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        if patch_size == 16:
            self.fpn1 = nn.Sequential(ConvTranspose2x2(embed_dim, embed_dim),
                                      build_norm_layer(dict(type="SyncBN"), embed_dim)[1], GELU(),
                                      ConvTranspose2x2(embed_dim, embed_dim))
            self.fpn2 = nn.Sequential(ConvTranspose2x2(embed_dim, embed_dim))
            self.fpn3 = nn.Identity()
            self.fpn4 = MaxPool(2)
        else:
            self.fpn1 = nn.Sequential(ConvTranspose2x2(embed_dim, embed_dim))
            self.fpn2 = nn.Identity()
            self.fpn3 = nn.Sequential(MaxPool(2))
            self.fpn4 = nn.Sequential(MaxPool(4))
        self._init_linears()
        self.fix_init_weight()

    def _init_linears(self):
        for m in self.modules():
            if isinstance(m, DynamicLinear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def fix_init_weight(self):
        with torch.no_grad():
            for layer_id, layer in enumerate(self.blocks):
                layer.attn.proj.weight.div_(math.sqrt(2.0 * (layer_id + 1)))
                layer.mlp.fc2.weight.div_(math.sqrt(2.0 * (layer_id + 1)))

    def init_weights(self, pretrained=None):
        """The constructor has initialised everything; a path loads that checkpoint on top (tables and
        position embeddings of another size are refused, not interpolated)."""
        if isinstance(pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)
        elif pretrained is not None:
            raise TypeError("pretrained must be a str or None")

    def get_num_layers(self):
        return len(self.blocks)

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def train(self, mode=True):
        """eval mode whatever is asked for: fpn1's BatchNorm always uses its running statistics"""
        return super().train(False)

    # ---- execution ----
    def _zero_pos(self, n, dev):
        """the position buffer of gs_vit_tokens_forward when there is no pos_embed: zeros, made once"""
        z = self.__dict__.get("_zero_pos_buf")
        if z is None or z.device != dev or z.shape[1] != n:
            z = self.__dict__["_zero_pos_buf"] = torch.zeros(1, n, self.embed_dim, device=dev)
        return z

    def forward_act(self, tape, img):
        if tape.enabled and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(FORWARD_ONLY)
        patches = self.patch_embed.forward_act(tape, img)
        hp, wp = patches.H, patches.W
        n = hp * wp + 1
        pos = self.pos_embed if self.pos_embed is not None else self._zero_pos(n, patches.t.device)
        x = ops.vit_tokens(tape, patches, self.cls_token, pos)
        shared = self.rel_pos_bias.relative_position_bias_table.detach() if self.rel_pos_bias is not None \
            else None
        features = []
        for i, blk in enumerate(self.blocks):
            table = blk.attn.relative_position_bias_table
            if table is None:
                table = shared
            elif shared is not None:
                table = table.detach() + shared   # both are added in the reference; the tables are tiny
            x = blk.forward_act(tape, x, table, (hp, wp))
            if i in self.out_indices:
                features.append(ops.vit_feature_map(tape, x, hp, wp))
        return [_run(tape, op, f) for op, f in zip((self.fpn1, self.fpn2, self.fpn3, self.fpn4), features)]

    def forward_features(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(FORWARD_ONLY)
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], False))

    def forward(self, x):
        return self.forward_features(x)
