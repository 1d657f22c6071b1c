"""ElasticTransformer backbone — host-side mirror of gaiaseg/models/backbones/elastic_transformer.py.

Same registered name, constructor signature, attribute and state-dict names and search space.  ``forward``
returns logical NCHW feature maps [B, D, H/patch, W/patch] (the cls row removed) and runs the whole
backbone as ONE autograd node over hand-written HIP kernels: the patch embedding and every linear on
gs_conv2d_*, the token assembly on gs_vit_tokens_*, LayerNorm and GELU on csrc/convnext_ops.hip and
multi-head self-attention on gs_attention_* (csrc/attention.hip).  Tokens travel as NHWC activations
[B, 1, N, D]; Q, K and V are three column slices of one buffer that the three linears write in place, and
the attention kernels read head h in columns [64 h, 64 h + 64) of each, so the reference's views, transposes
and ``.contiguous()`` calls have no counterpart here.

The search space is ``embedding`` ({'embed_dim': D}) and ``encoder`` (per encoder group the number of
layers, the number of heads and the feed-forward ratio r, hidden width int(r / 10 * D)), in the reference's
nested wire format.  Two departures from the reference, both on purpose:

* its ``manipulate_feedforward_channels`` overwrites the ratio inside the meta it is handed with the width,
  so a second call with the same meta gives another subnet; here metas are only read;
* it computes the hidden width from the embedding width of the PREVIOUS ``manipulate_embedding`` when the
  encoder key happens to be handled first; here the hidden width follows the current embedding width
  whichever key comes first.

Carried over as they are: the relative-position tables of every attention module and the final ``ln1`` are
parameters the reference creates and never uses (``relative_position`` is never turned on and the final
norm's call is commented out).  They stay in the state dict and out of ``active_modules()``.

Refused: ``drop_path > 0`` (stochastic depth), ``relative_position=True``, ``attn_drop`` / ``proj_drop`` /
``drop_rate > 0``, and an input whose size is not ``img_size`` (the reference asserts that too;
``pos_embed`` is not resized at forward time).
"""
import torch
import torch.nn as nn

from ...core.bricks import (DynamicLinear, build_activation_layer, build_conv_layer, build_norm_layer,
                            kaiming_init)
from ...core.dynamic import DynamicMixin
from ...hip import ops, streams
from ...hip.runtime import Act, tape_function
from ..builder import BACKBONES

HEAD_DIM = 64


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _refuse_positive(**kwargs):
    for key, value in kwargs.items():
        if value and value > 0:
            raise NotImplementedError("%s > 0 is not implemented (set %s=0)" % (key, key))


def _leaf(meta, key):
    """{'key': {'key': v}} or {'key': v} or v -> v: the value under the reference's nested meta"""
    while isinstance(meta, dict):
        meta = meta[key]
    return meta


def _nest(key, value):
    return {key: {key: value}}


def ffn_width(ratio, embed_dim):
    """hidden width of the feed-forward block for ratio ``ratio`` (tenths of the embedding width)"""
    return int(ratio / 10 * embed_dim)


class ElasticRelativePosition2D(nn.Module, DynamicMixin):
    """The two embedding tables of the reference's 2-D relative position; never read (see the module
    docstring), kept for the state dict."""

    def __init__(self, max_relative_position, num_units=64):
        super().__init__()
        self.num_units, self.max_relative_position = num_units, max_relative_position
        self.embeddings_table_v = nn.Parameter(torch.randn(max_relative_position * 2 + 2, num_units))
        self.embeddings_table_h = nn.Parameter(torch.randn(max_relative_position * 2 + 2, num_units))
        nn.init.normal_(self.embeddings_table_v, std=0.02)
        nn.init.normal_(self.embeddings_table_h, std=0.02)


class ElasticMHA(nn.Module, DynamicMixin):
    """x + proj(softmax(scale * Q K^T) V) with ``num_heads`` active heads of width 64."""
    search_space = {"num_heads"}
    fp16_attention = False   # set through ElasticTransformer.fp16_attention

    def __init__(self, embed_dim, num_heads, proj_drop=0.0, attn_drop=0.0, drop_path=0.1,
                 relative_position=False, max_relative_position=14):
        super().__init__()
        _refuse_positive(proj_drop=proj_drop, attn_drop=attn_drop, drop_path=drop_path)
        if relative_position:
            raise NotImplementedError("relative_position=True is not implemented (the reference never turns "
                                      "it on)")
        self.embed_dim, self.num_heads, self.max_heads = embed_dim, num_heads, num_heads
        self.w_ks = DynamicLinear(embed_dim, num_heads * HEAD_DIM)
        self.w_qs = DynamicLinear(embed_dim, num_heads * HEAD_DIM)
        self.w_vs = DynamicLinear(embed_dim, num_heads * HEAD_DIM)
        self.scale = HEAD_DIM ** -0.5
        self.proj = DynamicLinear(num_heads * HEAD_DIM, embed_dim)
        self.relative_position = relative_position
        self.max_relative_position = max_relative_position
        self.rel_pos_embed_k = ElasticRelativePosition2D(max_relative_position, HEAD_DIM)
        self.rel_pos_embed_v = ElasticRelativePosition2D(max_relative_position, HEAD_DIM)

    def manipulate_num_heads(self, arch_meta):
        heads = _leaf(arch_meta, "num_heads")
        if not 0 < heads <= self.max_heads:
            raise ValueError("num_heads %s out of range (1..%d)" % (heads, self.max_heads))
        self.num_heads_state = arch_meta
        self.num_heads = heads
        for lin in (self.w_ks, self.w_qs, self.w_vs):
            lin.manipulate_width(heads * HEAD_DIM)

    def active_children(self):
        return [self.w_ks, self.w_qs, self.w_vs, self.proj]

    def forward_act(self, tape, x, residual):
        width = self.num_heads * HEAD_DIM
        qkv = Act.empty(x.N, 1, x.W, 3 * width, x.t.device)
        q, k, v = (qkv.slice(i * width, (i + 1) * width) for i in range(3))
        self.w_qs.forward_act(tape, x, out=q)
        self.w_ks.forward_act(tape, x, out=k)
        self.w_vs.forward_act(tape, x, out=v)
        out = ops.attention(tape, q, k, v, self.num_heads, self.scale, f16=self.fp16_attention)
        self.proj.manipulate_width(residual.C)
        out = self.proj.forward_act(tape, out)
        return ops.layer_scale_add(tape, residual, out, None)


class ElasticFFN(nn.Module, DynamicMixin):
    """x + layer2(GELU(layer1(x)))"""
    search_space = {"feedforward_channels"}

    def __init__(self, embed_dim, feedforward_channels, num_fcs=2, act_cfg=dict(type="GELU"), drop_path=0.1,
                 dropout=0.0, add_residual=True):
        super().__init__()
        _refuse_positive(drop_path=drop_path, proj_drop=dropout)
        if num_fcs != 2 or not add_residual:
            raise NotImplementedError("ElasticFFN: two layers with the residual, as the reference builds it")
        self.embed_dim, self.feedforward_channels, self.num_fcs = embed_dim, feedforward_channels, num_fcs
        self.act_cfg = act_cfg
        self.activate = build_activation_layer(act_cfg)
        self.layer1 = DynamicLinear(embed_dim, feedforward_channels)
        self.layer2 = DynamicLinear(feedforward_channels, embed_dim)
        self.add_residual = add_residual

    def manipulate_feedforward_channels(self, arch_meta):
        """the hidden WIDTH (the encoder has turned the ratio into it)"""
        width = _leaf(arch_meta, "feedforward_channels")
        if width % 4:
            raise ValueError("feedforward_channels: the hidden width %d is no multiple of 4 (choose the ratio "
                             "so that int(ratio / 10 * embed_dim) is one)" % width)
        self.feedforward_channels_state = arch_meta
        self.layer1.manipulate_width(width)

    def forward_act(self, tape, x, residual):
        out = self.layer1.forward_act(tape, x)
        out = self.activate.forward_act(tape, out)
        self.layer2.manipulate_width(residual.C)
        out = self.layer2.forward_act(tape, out)
        return ops.layer_scale_add(tape, residual, out, None)


class ElasticTransformerEncoderLayer(nn.Module, DynamicMixin):
    def __init__(self, embed_dim, num_heads, feedforward_channels, attn_drop=0.0, proj_drop=0.0, drop_path=0.1,
                 act_cfg=dict(type="GELU"), norm_cfg=dict(type="ElaLN"), num_fcs=2):
        super().__init__()
        _refuse_positive(attn_drop=attn_drop)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, embed_dim, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.attn = ElasticMHA(embed_dim=embed_dim, num_heads=num_heads, proj_drop=0.0, attn_drop=0.0,
                               drop_path=drop_path)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, embed_dim, postfix=2)
        self.add_module(self.norm2_name, norm2)
        self.mlp = ElasticFFN(embed_dim=embed_dim, feedforward_channels=feedforward_channels, num_fcs=num_fcs,
                              act_cfg=act_cfg, drop_path=drop_path, dropout=proj_drop)

    norm1 = property(lambda self: getattr(self, self.norm1_name))
    norm2 = property(lambda self: getattr(self, self.norm2_name))

    def forward_act(self, tape, x):
        x = self.attn.forward_act(tape, self.norm1.forward_act(tape, x), residual=x)
        return self.mlp.forward_act(tape, self.norm2.forward_act(tape, x), residual=x)


class ElasticEncoder(nn.ModuleList, DynamicMixin):
    """One encoder group: ``num_layers`` layers at their maximum size, only the first ``num_layers_state``
    run, all at the group's head count and feed-forward ratio."""
    search_space = {"num_layers", "embed_dim", "num_heads", "feedforward_channels"}

    def __init__(self, embed_dim, num_heads, feedforward_channels, num_layers, attn_drop=0.0, proj_drop=0.0,
                 drop_path=0.0, act_cfg=dict(type="GELU"), norm_cfg=dict(type="ElaLN"), num_fcs=2):
        if not isinstance(drop_path, (list, tuple)):
            drop_path = [drop_path] * num_layers
        super().__init__([ElasticTransformerEncoderLayer(
            embed_dim=embed_dim, num_heads=num_heads, feedforward_channels=feedforward_channels,
            attn_drop=attn_drop, proj_drop=proj_drop, drop_path=drop_path[i], act_cfg=act_cfg,
            norm_cfg=norm_cfg, num_fcs=num_fcs) for i in range(num_layers)])
        self.embed_dim_state = embed_dim
        self.init_state(num_layers=num_layers, num_heads=_nest("num_heads", num_heads),
                        feedforward_channels=_nest("feedforward_channels", feedforward_channels))
        self._ratio = None   # the feed-forward ratio, once one has been set

    def manipulate_num_layers(self, arch_meta):
        assert arch_meta >= 1, "Depth must be greater than 0, skipping stage is not supported yet."
        if arch_meta > len(self):
            raise ValueError("num_layers %d exceeds the %d layers of this encoder" % (arch_meta, len(self)))
        self.num_layers_state = arch_meta

    def manipulate_embed_dim(self, arch_meta):
        self.embed_dim_state = arch_meta
        self._apply_ratio()

    def manipulate_num_heads(self, arch_meta):
        self.num_heads_state = arch_meta
        for m in self:   # every layer, skipped ones included, as in the reference
            m.attn.manipulate_arch(arch_meta)

    def manipulate_feedforward_channels(self, arch_meta):
        self.feedforward_channels_state = arch_meta
        self._ratio = _leaf(arch_meta, "feedforward_channels")
        self._apply_ratio()

    def _apply_ratio(self):
        if self._ratio is None:
            return
        width = ffn_width(self._ratio, self.embed_dim_state)
        for m in self:
            m.mlp.manipulate_arch(_nest("feedforward_channels", width))

    def active_layers(self):
        return [self[i] for i in range(self.num_layers_state)]

    def forward_act(self, tape, x, extra_out_indices=None):
        if getattr(self, "_deploying", False):
            del self[self.num_layers_state:]
        outputs = []
        for i in range(self.num_layers_state):
            x = self[i].forward_act(tape, x)
            if extra_out_indices is not None and i in extra_out_indices:
                outputs.append(x)
        if extra_out_indices is not None:
            outputs.append(x)
            return outputs
        return x


class ElasticPatchEmbed(nn.Module, DynamicMixin):
    def __init__(self, embed_dim, img_size=224, patch_size=16, in_channels=3,
                 conv_cfg=dict(type="ElasticConv2d")):
        super().__init__()
        self.img_size, self.patch_size = _pair(img_size), _pair(patch_size)
        if self.patch_size[0] != self.patch_size[1]:
            raise NotImplementedError("patch_size: only square patches")
        self.num_patches = (self.img_size[1] // self.patch_size[1]) * (self.img_size[0] // self.patch_size[0])
        self.projection = build_conv_layer(conv_cfg, in_channels, embed_dim, kernel_size=self.patch_size[0],
                                           stride=self.patch_size[0])
        self.init_weights()

    def init_weights(self):
        kaiming_init(self.projection, mode="fan_in", nonlinearity="linear")

    def forward_act(self, tape, x):
        h, w = (x.t.shape[2], x.t.shape[3]) if x.nchw_image else (x.H, x.W)
        if (h, w) != self.img_size:
            raise ValueError("img_size: input image size (%d*%d) doesn't match model (%d*%d)"
                             % (h, w, self.img_size[0], self.img_size[1]))
        return self.projection.forward_act(tape, x)


@BACKBONES.register_module()
class ElasticTransformer(nn.Module, DynamicMixin):
    """Vision transformer with an elastic embedding width and, per encoder group, elastic depth, head
    count and feed-forward ratio."""
    search_space = {"embedding", "encoder"}
    _fp16_attention = False

    def __init__(self, embed_dim, num_heads, feedforward_channels, num_layers, patch_size=16, img_size=224,
                 in_channels=3, attn_drop=0.0, proj_drop=0.0, drop_rate=0.0, drop_path=0.1,
                 norm_cfg=dict(type="ElaLN"), act_cfg=dict(type="GELU"), num_fcs=2, out_indices=None,
                 out_stages=None, init_cfg=None, pretrained=None, interpolate_mode="bicubic"):
        super().__init__()
        assert not (init_cfg and pretrained), "init_cfg and pretrained cannot be set at the same time"
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        _refuse_positive(drop_path=drop_path, attn_drop=attn_drop, proj_drop=proj_drop, drop_rate=drop_rate)
        if len(num_layers) != 3:
            raise AssertionError("ElasticTransformer has three encoder groups: num_layers needs three entries")
        if not isinstance(patch_size, int):
            raise NotImplementedError("patch_size: an int, as the reference's forward requires")
        self.embed_dim, self.num_heads, self.feedforward_channels = embed_dim, num_heads, feedforward_channels
        self.num_layers, self.patch_size, self.img_size = list(num_layers), patch_size, img_size
        self.init_cfg = init_cfg
        self.elastic_patch_embed = ElasticPatchEmbed(img_size=img_size, patch_size=patch_size,
                                                     in_channels=in_channels, embed_dim=embed_dim)
        num_patches = self.elastic_patch_embed.num_patches
        self.interpolate_mode = interpolate_mode
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.init_state(embedding={"embed_dim": embed_dim},
                        encoder={"num_layers": list(num_layers),
                                 "num_heads": _nest("num_heads", [num_heads] * 3),
                                 "feedforward_channels": _nest("feedforward_channels",
                                                               [feedforward_channels] * 3)})
        self.layers = []
        for i, num_layer in enumerate(self.num_layers):
            name = "elastic_encoder%d" % (i + 1)
            self.add_module(name, self.make_encoder(
                embed_dim=embed_dim, num_heads=num_heads, feedforward_channels=feedforward_channels,
                num_layers=num_layer, attn_drop=attn_drop, proj_drop=proj_drop, drop_path=[0.] * num_layer,
                act_cfg=act_cfg, norm_cfg=norm_cfg, num_fcs=num_fcs))
            self.layers.append(name)
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, embed_dim, postfix=1)
        self.add_module(self.norm1_name, norm1)
        self.out_indices = out_indices if out_indices is not None else [None] * 3
        self.out_stages = out_stages if out_stages is not None else [2]
        self.init_weights(pretrained)

    norm1 = property(lambda self: getattr(self, self.norm1_name))

    @property
    def fp16_attention(self):
        """Opt-in (core.fp16_utils.wrap_fp16_model(model, attention=True); ``fp16 = dict(attention=True)``
        in a config): inside an fp16 mode every attention runs on the fp16-operand kernels
        (ops.attention(f16=True)).  Without an fp16 mode the flag does nothing."""
        return self._fp16_attention

    @fp16_attention.setter
    def fp16_attention(self, flag):
        self._fp16_attention = bool(flag)
        for m in self.modules():
            if isinstance(m, ElasticMHA):
                m.fp16_attention = self._fp16_attention

    def make_encoder(self, **kwargs):
        return ElasticEncoder(**kwargs)

    def init_weights(self, pretrained=None):
        """The reference's non-pretrained branch: truncated normal (std 0.02) linears with zero biases,
        tokens and position embedding; kaiming fan-in for the patch conv; unit LayerNorms.  Then the
        checkpoint, if a path is given (position embeddings are not resized)."""
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, DynamicLinear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)
        kaiming_init(self.elastic_patch_embed.projection, mode="fan_in", bias=0.)
        if isinstance(pretrained, str):
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(self, pretrained, strict=False)

    # ---- arch manipulation ----
    def manipulate_embedding(self, arch_meta):
        self.embedding_state = arch_meta
        d = arch_meta["embed_dim"]
        if d % 4 or not 0 < d <= self.embed_dim:
            raise ValueError("embed_dim %s: a multiple of 4 in 4..%d" % (d, self.embed_dim))
        self.elastic_patch_embed.projection.manipulate_width(d)
        for name in self.layers:
            getattr(self, name).manipulate_arch(arch_meta)

    def manipulate_encoder(self, arch_meta):
        """{'num_layers': [3], 'num_heads': {'num_heads': {'num_heads': [3]}}, 'feedforward_channels':
        {'feedforward_channels': {'feedforward_channels': [3 ratios]}}}; the meta is only read."""
        self.encoder_state = arch_meta
        layers = arch_meta["num_layers"]
        heads, ratios = _leaf(arch_meta["num_heads"], "num_heads"), \
            _leaf(arch_meta["feedforward_channels"], "feedforward_channels")
        for i, name in enumerate(self.layers):
            getattr(self, name).manipulate_arch({
                "num_layers": layers[i], "num_heads": _nest("num_heads", heads[i]),
                "feedforward_channels": _nest("feedforward_channels", ratios[i])})

    def full_arch_meta(self):
        """the largest architecture of this supernet, in the form manipulate_arch takes"""
        ratio = round(10 * self.feedforward_channels / self.embed_dim)
        if ffn_width(ratio, self.embed_dim) != self.feedforward_channels:
            raise ValueError("feedforward_channels %d is not int(ratio / 10 * %d) for an integer ratio"
                             % (self.feedforward_channels, self.embed_dim))
        return {"embedding": {"embed_dim": self.embed_dim},
                "encoder": {"num_layers": list(self.num_layers),
                            "num_heads": _nest("num_heads", [self.num_heads] * 3),
                            "feedforward_channels": _nest("feedforward_channels", [ratio] * 3)}}

    # ---- execution ----
    def forward_act(self, tape, img):
        patches = self.elastic_patch_embed.forward_act(tape, img)
        hp, wp, d = patches.H, patches.W, patches.C
        if getattr(self, "_deploying", False) and self.cls_token.shape[-1] != d:
            self.cls_token = nn.Parameter(self.cls_token.data[..., :d].clone(), self.cls_token.requires_grad)
            self.pos_embed = nn.Parameter(self.pos_embed.data[..., :d].clone(), self.pos_embed.requires_grad)
            self.norm1._deploy_slice(d)
        x = ops.vit_tokens(tape, patches, self.cls_token, self.pos_embed)
        outputs = []
        for i, name in enumerate(self.layers):
            x = getattr(self, name).forward_act(tape, x, self.out_indices[i])
            if i == 0:
                streams.side_checkpoint(tape)   # as the other backbones: later layers' gradients are ready first
            if i in self.out_stages:
                outputs.extend(x if isinstance(x, list) else [x])
            if isinstance(x, list):
                x = x[-1]
        return [ops.vit_feature_map(tape, o, hp, wp) for o in outputs]

    def forward(self, x):
        needs = any(p.requires_grad for p in self.parameters())
        return tuple(tape_function(lambda tape, acts: self.forward_act(tape, acts[0]), [x], needs))

    def late_gradient_parameters(self):
        """Parameters whose gradients are produced after the side-stream checkpoint (patch embedding,
        tokens, first encoder group)."""
        params = [self.cls_token, self.pos_embed] + list(self.elastic_patch_embed.parameters())
        for layer in getattr(self, self.layers[0]).active_layers():
            params += [p for m in _layer_active_modules(layer) for p in m.parameters()]
        return params

    def active_modules(self):
        """Modules whose parameters take part in the current subnet: the patch embedding, the tokens and
        the active layers' norms, linears; not the skipped layers, the relative-position tables or the
        final ``ln1``."""
        mods = [self.elastic_patch_embed, _Tokens(self)]
        for name in self.layers:
            for layer in getattr(self, name).active_layers():
                mods.extend(_layer_active_modules(layer))
        return mods


def _layer_active_modules(layer):
    return [layer.norm1, layer.norm2, layer.mlp.layer1, layer.mlp.layer2] + layer.attn.active_children()


class _Tokens:
    """cls_token and pos_embed as a 'module' of active_modules(): they are parameters of the backbone
    itself, whose other direct parameters (none) and unused children must not come along."""

    def __init__(self, backbone):
        self._params = [backbone.cls_token, backbone.pos_embed]

    def parameters(self):
        return iter(self._params)
