"""float64 CPU references for the attention operator, the ViT token assembly and the ElasticTransformer
backbone, written from the maths and torch's own operators (softmax, F.layer_norm, F.gelu, F.linear,
F.conv2d).  Token tensors are "rows x C" views [B, N, C] with head h in columns [64 h, 64 h + 64), like the
kernels' operands."""
import torch
import torch.nn.functional as F

HEAD_DIM = 64
SCALE = HEAD_DIM ** -0.5


# ---- operator cases --------------------------------------------------------------------------------------
T = 128   # the larger of the kernels' tiles: a workgroup owns 128 query rows (the swept tile is 32 rows)
# (name, B, N, heads, sliced operands?, dominant key?)
ATTENTION_CASES = [
    ("single-token", 1, 1, 1, False, False),
    ("below-one-tile", 2, 17, 1, False, False),
    ("one-tile", 2, T, 2, False, False),
    ("ragged-by-one", 2, T + 1, 3, False, False),
    ("sliced-4th-head-idle", 1, 2 * T + 9, 3, True, False),
    ("late-dominant-key", 1, 2 * T + 9, 3, False, True),
]


def attention_inputs(b, n, heads, dominant, seed, dtype=torch.float32):
    """q, k, v, dO, and the bases an accumulating backward adds to: [b, n, 64 * heads] each.  ``dominant``:
    in every head the first component of every second query is 8 and that of the LAST key (it lies in the
    last, ragged tile) is 30 / (scale * 8) = 30, so for those queries the last key's score is 30 above the
    N(0, 1) scores of the others: the running maximum moves in the last tile and everything summed before
    is rescaled by about e^-30.  The other queries keep O(1) probabilities everywhere, which keeps the
    gradients' largest elements (what rel_err divides by) well conditioned in fp32."""
    g = torch.Generator().manual_seed(seed)
    c = HEAD_DIM * heads
    q, k, v, do, bq, bk, bv = (torch.randn(b, n, c, generator=g) for _ in range(7))
    if dominant:
        q[:, ::2, ::HEAD_DIM] = 8.0
        k[:, -1, ::HEAD_DIM] = 30.0 / (SCALE * 8.0)
    return tuple(t.to(dtype) for t in (q, k, v, do, bq, bk, bv))


def attention_formula(q, k, v, heads, scale=SCALE):
    """softmax(scale * Q K^T) V per head, in the dtype of the inputs: [b, n, 64 * heads] -> (O, lse)"""
    b, n, _ = q.shape
    qh, kh, vh = (t.view(b, n, heads, HEAD_DIM).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-2, -1)) * scale
    o = s.softmax(dim=-1) @ vh
    return o.transpose(1, 2).reshape(b, n, heads * HEAD_DIM), torch.logsumexp(s, dim=-1)


def attention_ref(q, k, v, do, heads, scale=SCALE):
    """float64 -> (O, lse [b, heads, n], dQ, dK, dV)"""
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    o, lse = attention_formula(qr, kr, vr, heads, scale)
    o.backward(do.double())
    return o.detach(), lse.detach(), qr.grad, kr.grad, vr.grad


def attention_fp32(q, k, v, do, heads, scale=SCALE):
    """the same formula in float32 torch on the CPU (the input-conditioning check)"""
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o, lse = attention_formula(qr, kr, vr, heads, scale)
    o.backward(do.float())
    return o.detach(), lse.detach(), qr.grad, kr.grad, vr.grad


def tokens_ref(patches, cls, pos, dx):
    """patches [b, t, d], cls [d], pos [t + 1, d], dx [b, t + 1, d] -> (x, dpatches, dcls, dpos), float64"""
    p, c, e = (t.double().requires_grad_(True) for t in (patches, cls, pos))
    x = torch.cat([c.expand(p.shape[0], 1, -1), p], dim=1) + e
    x.backward(dx.double())
    return x.detach(), p.grad, c.grad, e.grad


# ---- the backbone ----------------------------------------------------------------------------------------
TINY = dict(embed_dim=128, num_heads=2, feedforward_channels=512, num_layers=[1, 2, 1], img_size=(32, 48),
            patch_size=16)
# embed_dim, heads / layers / feed-forward ratios per encoder group
SUBNETS = {"max": dict(embed_dim=128, heads=[2, 2, 2], layers=[1, 2, 1], ratios=[40, 40, 40]),
           "sub": dict(embed_dim=64, heads=[1, 2, 1], layers=[1, 1, 1], ratios=[30, 40, 35])}
OUT_INDICES = [None, [0], None]   # group 2 also hands out its first layer: four feature maps
OUT_STAGES = [0, 1, 2]
NECK_SCALES = [4, 2, 1, 1]        # a 2 x 3 token grid has no exact half


def tiny_backbone_cfg(**kw):
    cfg = dict(type="ElasticTransformer", drop_path=0.0, out_indices=[None if i is None else list(i)
                                                                      for i in OUT_INDICES],
               out_stages=list(OUT_STAGES), **{k: (list(v) if isinstance(v, list) else v) for k, v in TINY.items()})
    cfg.update(kw)
    return cfg


def tiny_model_cfg():
    """DynamicUPerHead over DynamicMultiLevelNeck over the tiny ElasticTransformer, FCN auxiliary head"""
    from util_models import fcn_head, uper_head
    d = TINY["embed_dim"]
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(),
                neck=dict(type="DynamicMultiLevelNeck", in_channels=[d] * 4, out_channels=16,
                          scales=list(NECK_SCALES), conv_cfg=dict(type="DynConv2d")),
                decode_head=uper_head(in_channels=[16] * 4, channels=16),
                auxiliary_head=fcn_head(in_channels=16, in_index=2, channels=16, num_convs=1,
                                        concat_input=False, loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def nest(key, value):
    return {key: {key: value}}


def arch_of(name):
    """the arch of a subnet in the form ElasticTransformer.manipulate_arch takes"""
    a = SUBNETS[name]
    return {"embedding": {"embed_dim": a["embed_dim"]},
            "encoder": {"num_layers": list(a["layers"]), "num_heads": nest("num_heads", list(a["heads"])),
                        "feedforward_channels": nest("feedforward_channels", list(a["ratios"]))}}


def arch_meta(name):
    """the same as a flat sampler meta"""
    a = SUBNETS[name]
    enc = "arch.backbone.encoder."
    return {"name": name, "arch.backbone.embedding.embed_dim": a["embed_dim"],
            enc + "num_layers": list(a["layers"]),
            enc + "num_heads.num_heads.num_heads": list(a["heads"]),
            enc + "feedforward_channels.feedforward_channels.feedforward_channels": list(a["ratios"])}


def ffn_width(ratio, d):
    return int(ratio / 10 * d)


def randomize_vit(backbone, seed=0):
    """O(1) LayerNorm affines, tokens and biases, weights that keep activations O(1)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if ".ln" in "." + name and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
            elif "embeddings_table" in name or name in ("cls_token", "pos_embed"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            else:
                raise AssertionError("unexpected parameter %s %s" % (name, tuple(p.shape)))


def vit_ref(sd, x, arch, eps=1e-5, out_indices=OUT_INDICES, out_stages=OUT_STAGES, patch=16):
    """The ElasticTransformer on float64 tensors for a state dict of max-size tensors ``sd`` (2-D linear
    weights) and the subnet ``arch`` (an entry of SUBNETS): leading slices of every parameter, the first
    layers[i] layers of group i.  Returns the feature maps [B, D, H / patch, W / patch]."""
    d = arch["embed_dim"]
    b, _, h, w = x.shape
    t = F.conv2d(x, sd["elastic_patch_embed.projection.weight"][:d], sd["elastic_patch_embed.projection.bias"][:d],
                 stride=patch).flatten(2).transpose(1, 2)
    n = t.shape[1] + 1
    t = torch.cat([sd["cls_token"][:, :, :d].expand(b, -1, -1), t], dim=1) + sd["pos_embed"][:, :n, :d]

    def lin(v, name, co):
        return F.linear(v, sd[name + ".weight"][:co, :v.shape[-1]], sd[name + ".bias"][:co])

    def ln(v, name):
        return F.layer_norm(v, (d,), sd[name + ".weight"][:d], sd[name + ".bias"][:d], eps)

    outs = []
    for i in range(3):
        heads, hidden = arch["heads"][i], ffn_width(arch["ratios"][i], d)
        group = []
        for j in range(arch["layers"][i]):
            p = "elastic_encoder%d.%d." % (i + 1, j)
            y = ln(t, p + "ln1")
            o, _ = attention_formula(lin(y, p + "attn.w_qs", 64 * heads), lin(y, p + "attn.w_ks", 64 * heads),
                                     lin(y, p + "attn.w_vs", 64 * heads), heads)
            t = t + lin(o, p + "attn.proj", d)
            t = t + lin(F.gelu(lin(ln(t, p + "ln2"), p + "mlp.layer1", hidden)), p + "mlp.layer2", d)
            if out_indices[i] is not None and j in out_indices[i]:
                group.append(t)
        if out_indices[i] is not None:
            group.append(t)
        else:
            group = [t]
        if i in out_stages:
            outs.extend(group)
    return [o[:, 1:].reshape(b, h // patch, w // patch, d).permute(0, 3, 1, 2) for o in outs]


def active_slice(name, arch, n_tokens):
    """index of the part of state-dict tensor ``name`` that subnet ``arch`` reads, or None where it reads
    nothing of it (a skipped layer, the relative-position tables, the final ln1)"""
    d = arch["embed_dim"]
    if name == "cls_token":
        return (slice(None), slice(None), slice(0, d))
    if name == "pos_embed":
        return (slice(None), slice(0, n_tokens), slice(0, d))
    if name.startswith("elastic_patch_embed.projection."):
        return (slice(0, d),)
    if not name.startswith("elastic_encoder") or "rel_pos_embed" in name:
        return None
    group, layer, rest = name[len("elastic_encoder"):].split(".", 2)
    i = int(group) - 1
    if int(layer) >= arch["layers"][i]:
        return None
    hw, hidden = 64 * arch["heads"][i], ffn_width(arch["ratios"][i], d)
    mod, kind = rest.rsplit(".", 1)
    out, inp = {"ln1": (d, None), "ln2": (d, None), "attn.w_qs": (hw, d), "attn.w_ks": (hw, d),
                "attn.w_vs": (hw, d), "attn.proj": (d, hw), "mlp.layer1": (hidden, d), "mlp.layer2": (d, hidden)}[mod]
    return (slice(0, out), slice(0, inp)) if kind == "weight" and inp is not None else (slice(0, out),)


def vit_param_names(embed_dim, num_heads, ffn, num_layers, n_tokens, patch=16, in_channels=3, max_rel=14):
    """state-dict names and shapes of an ElasticTransformer, in order (closed form of the constructor)"""
    out = [("cls_token", (1, 1, embed_dim)), ("pos_embed", (1, n_tokens, embed_dim)),
           ("elastic_patch_embed.projection.weight", (embed_dim, in_channels, patch, patch)),
           ("elastic_patch_embed.projection.bias", (embed_dim,))]
    hw = 64 * num_heads
    for i, layers in enumerate(num_layers):
        for j in range(layers):
            p = "elastic_encoder%d.%d." % (i + 1, j)
            out += [(p + "ln1.weight", (embed_dim,)), (p + "ln1.bias", (embed_dim,))]
            for lin in ("w_ks", "w_qs", "w_vs"):
                out += [(p + "attn.%s.weight" % lin, (hw, embed_dim)), (p + "attn.%s.bias" % lin, (hw,))]
            out += [(p + "attn.proj.weight", (embed_dim, hw)), (p + "attn.proj.bias", (embed_dim,))]
            for tab in ("k", "v"):
                out += [(p + "attn.rel_pos_embed_%s.embeddings_table_v" % tab, (2 * max_rel + 2, 64)),
                        (p + "attn.rel_pos_embed_%s.embeddings_table_h" % tab, (2 * max_rel + 2, 64))]
            out += [(p + "ln2.weight", (embed_dim,)), (p + "ln2.bias", (embed_dim,)),
                    (p + "mlp.layer1.weight", (ffn, embed_dim)), (p + "mlp.layer1.bias", (ffn,)),
                    (p + "mlp.layer2.weight", (embed_dim, ffn)), (p + "mlp.layer2.bias", (embed_dim,))]
    return out + [("ln1.weight", (embed_dim,)), ("ln1.bias", (embed_dim,))]
