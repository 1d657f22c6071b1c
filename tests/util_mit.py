"""float64 CPU references for attention with separate query and key lengths (gs_attention_kv_*) and for the
DynamicMixVisionTransformer backbone, written from the maths with torch's own operators (softmax,
F.layer_norm, F.gelu, F.linear, F.conv2d), like util_vit.py.  Token tensors are "rows x C" views [B, N, C]
with head h in columns [64 h, 64 h + 64)."""
import torch
import torch.nn.functional as F

from util_vit import HEAD_DIM, SCALE

# ---- operator cases --------------------------------------------------------------------------------------
# A workgroup owns 128 rows (queries in the forward and dQ, keys in dK / dV) and sweeps the others in tiles
# of 32.  (name, B, Nq, Nk, heads, sliced operands?, dominant last key?)
KV_CASES = [
    ("single", 1, 1, 1, 1, False, False),
    ("below-tiles", 2, 17, 5, 1, False, False),
    ("exact-tiles", 2, 128, 32, 2, False, False),
    ("ragged-by-one", 2, 129, 33, 3, False, False),
    ("keys-outnumber-queries", 1, 40, 265, 2, False, False),
    ("sliced-idle-4th-head", 1, 265, 40, 3, True, False),
    ("late-dominant-key", 1, 265, 41, 3, False, True),
]
SPLIT_CASE = (2, 300, 40, 2)   # ten query tiles, the last one ragged
SPLITS = (1, 2, 3, 10)


def kv_inputs(b, nq, nk, heads, dominant, seed, dtype=torch.float32):
    """q, k, v, dO and the bases an accumulating backward adds to: q, dO, bq are [b, nq, 64 * heads], k, v,
    bk, bv are [b, nk, 64 * heads].  ``dominant`` as util_vit.attention_inputs: the last key (in the last,
    ragged key tile) scores 30 above the others for every second query."""
    g = torch.Generator().manual_seed(seed)
    c = HEAD_DIM * heads
    q, do, bq = (torch.randn(b, nq, c, generator=g) for _ in range(3))
    k, v, bk, bv = (torch.randn(b, nk, c, generator=g) for _ in range(4))
    if dominant:
        q[:, ::2, ::HEAD_DIM] = 8.0
        k[:, -1, ::HEAD_DIM] = 30.0 / (SCALE * 8.0)
    return tuple(t.to(dtype) for t in (q, k, v, do, bq, bk, bv))


def kv_formula(q, k, v, heads, scale=SCALE):
    """softmax(scale * Q K^T) V per head, in the dtype of the inputs: q [b, nq, c], k, v [b, nk, c] ->
    (O [b, nq, c], lse [b, heads, nq])"""
    b, nq, _ = q.shape
    qh = q.view(b, nq, heads, HEAD_DIM).transpose(1, 2)
    kh, vh = (t.view(b, t.shape[1], heads, HEAD_DIM).transpose(1, 2) for t in (k, v))
    s = (qh @ kh.transpose(-2, -1)) * scale
    o = s.softmax(dim=-1) @ vh
    return o.transpose(1, 2).reshape(b, nq, heads * HEAD_DIM), torch.logsumexp(s, dim=-1)


def kv_ref(q, k, v, do, heads, scale=SCALE, dtype=torch.float64):
    """-> (O, lse, dQ, dK, dV) in ``dtype`` (float64: the reference; float32: the input-conditioning check)"""
    qr, kr, vr = (t.to(dtype).requires_grad_(True) for t in (q, k, v))
    o, lse = kv_formula(qr, kr, vr, heads, scale)
    o.backward(do.to(dtype))
    return o.detach(), lse.detach(), qr.grad, kr.grad, vr.grad


# ---- the backbone ----------------------------------------------------------------------------------------
# supernet maxima of the tiny backbone: width = 64 * heads
TINY = dict(num_layers=[1, 2, 1, 1], num_heads=[1, 2, 3, 2], sr_ratios=[8, 4, 2, 1], mlp_ratio=4)
PATCH_SIZES, STRIDES = (7, 3, 3, 3), (4, 2, 2, 2)
SUBNETS = {"max": dict(depth=[1, 2, 1, 1], num_heads=[1, 2, 3, 2], mlp_ratio=[4, 4, 4, 4]),
           "sub": dict(depth=[1, 1, 1, 1], num_heads=[1, 1, 2, 1], mlp_ratio=[2, 4, 3, 2])}
EPS = 1e-6


def tiny_backbone_cfg(**kw):
    cfg = dict(type="DynamicMixVisionTransformer", **{k: (list(v) if isinstance(v, list) else v)
                                                      for k, v in TINY.items()})
    cfg.update(kw)
    return cfg


def segformer_head_cfg(in_channels, channels=16, align_corners=False):
    from util_models import CONV
    return dict(type="DynamicSegformerHead", conv_cfg=CONV, in_channels=list(in_channels), in_index=[0, 1, 2, 3],
                channels=channels, dropout_ratio=0.0, num_classes=19, norm_cfg=dict(type="SyncBN", requires_grad=True),
                align_corners=align_corners,
                loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))


def tiny_model_cfg():
    """DynamicSegformerHead over the tiny DynamicMixVisionTransformer, FCN auxiliary head on level 2"""
    from util_models import fcn_head
    w = widths(SUBNETS["max"])
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(), decode_head=segformer_head_cfg(w),
                auxiliary_head=fcn_head(in_channels=w[2], in_index=2, channels=16, num_convs=1, concat_input=False,
                                        loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def arch_of(name):
    """the arch of a subnet in the form DynamicMixVisionTransformer.manipulate_arch takes"""
    return {"body": {k: list(v) for k, v in SUBNETS[name].items()}}


def arch_meta(name):
    """the same as a flat sampler meta"""
    return dict({"name": name}, **{"arch.backbone.body." + k: list(v) for k, v in SUBNETS[name].items()})


def widths(arch):
    return [HEAD_DIM * h for h in arch["num_heads"]]


def hidden_width(ratio, d):
    return int(ratio * d)


def randomize_mit(backbone, seed=0):
    """O(1) LayerNorm weights, small biases, weights that keep activations O(1)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) / fan_in ** 0.5)


def mit_ref(sd, x, arch, sr_ratios=TINY["sr_ratios"], eps=EPS):
    """The Mix Transformer encoder on the tensors of ``sd`` (max-size tensors under the names of
    transformers' SegformerModel encoder; 2-D linear weights) in the dtype of ``x`` for the subnet ``arch``
    (an entry of SUBNETS): leading slices of every parameter, the first depth[i] blocks of stage i.  Returns
    the four feature maps [B, D_i, H_i, W_i]."""
    outs = []
    for i in range(4):
        d, heads, depth = HEAD_DIM * arch["num_heads"][i], arch["num_heads"][i], arch["depth"][i]
        hidden, sr = hidden_width(arch["mlp_ratio"][i], d), sr_ratios[i]
        p = "stages.%d." % i

        def lin(v, name, co):
            return F.linear(v, sd[name + ".weight"][:co, :v.shape[-1]], sd[name + ".bias"][:co])

        def ln(v, name):
            return F.layer_norm(v, (d,), sd[name + ".weight"][:d], sd[name + ".bias"][:d], eps)

        x = F.conv2d(x, sd[p + "patch_embeddings.proj.weight"][:d, :x.shape[1]],
                     sd[p + "patch_embeddings.proj.bias"][:d], stride=STRIDES[i], padding=PATCH_SIZES[i] // 2)
        b, _, h, w = x.shape
        t = ln(x.flatten(2).transpose(1, 2), p + "patch_embeddings.layer_norm")
        for j in range(depth):
            q = p + "blocks.%d." % j
            y = ln(t, q + "layernorm_before")
            r = y
            if sr > 1:
                rp = q + "attention.sequence_reduction."
                r = F.conv2d(y.transpose(1, 2).reshape(b, d, h, w), sd[rp + "sequence_reduction.weight"][:d, :d],
                             sd[rp + "sequence_reduction.bias"][:d], stride=sr)
                r = ln(r.flatten(2).transpose(1, 2), rp + "layer_norm")
            o, _ = kv_formula(lin(y, q + "attention.q_proj", d), lin(r, q + "attention.k_proj", d),
                              lin(r, q + "attention.v_proj", d), heads)
            t = t + lin(o, q + "attention.o_proj", d)
            z = lin(ln(t, q + "layernorm_after"), q + "mlp.fc1", hidden)
            z = F.conv2d(z.transpose(1, 2).reshape(b, hidden, h, w), sd[q + "mlp.dwconv.dwconv.weight"][:hidden],
                         sd[q + "mlp.dwconv.dwconv.bias"][:hidden], padding=1, groups=hidden)
            t = t + lin(F.gelu(z.flatten(2).transpose(1, 2)), q + "mlp.fc2", d)
        t = ln(t, p + "layer_norm")
        x = t.transpose(1, 2).reshape(b, d, h, w)
        outs.append(x)
    return outs


def active_slice(name, arch):
    """index of the part of state-dict tensor ``name`` that subnet ``arch`` reads, or None where it reads
    nothing of it (a block past the stage's depth)"""
    parts = name.split(".")
    i = int(parts[1])
    d = HEAD_DIM * arch["num_heads"][i]
    d_in = 3 if i == 0 else HEAD_DIM * arch["num_heads"][i - 1]
    hidden = hidden_width(arch["mlp_ratio"][i], d)
    kind = parts[-1]
    if parts[2] == "patch_embeddings":
        return (slice(0, d), slice(0, d_in)) if parts[3] == "proj" and kind == "weight" else (slice(0, d),)
    if parts[2] == "layer_norm":
        return (slice(0, d),)
    if int(parts[3]) >= arch["depth"][i]:
        return None
    mod = ".".join(parts[4:-1])
    out, inp = {"layernorm_before": (d, None), "layernorm_after": (d, None), "attention.q_proj": (d, d),
                "attention.k_proj": (d, d), "attention.v_proj": (d, d), "attention.o_proj": (d, d),
                "attention.sequence_reduction.sequence_reduction": (d, d),
                "attention.sequence_reduction.layer_norm": (d, None), "mlp.fc1": (hidden, d),
                "mlp.dwconv.dwconv": (hidden, None), "mlp.fc2": (d, hidden)}[mod]
    return (slice(0, out), slice(0, inp)) if kind == "weight" and inp is not None else (slice(0, out),)


def hf_config(arch, sr_ratios=TINY["sr_ratios"]):
    """the transformers SegformerConfig of a net of exactly the sizes of subnet ``arch`` (mlp ratios must be
    integers there only in name: the hidden width is int(ratio * width))"""
    from transformers import SegformerConfig
    return SegformerConfig(num_channels=3, num_encoder_blocks=4, depths=list(arch["depth"]),
                           sr_ratios=list(sr_ratios), hidden_sizes=widths(arch),
                           patch_sizes=list(PATCH_SIZES), strides=list(STRIDES),
                           num_attention_heads=list(arch["num_heads"]), mlp_ratios=list(arch["mlp_ratio"]),
                           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, classifier_dropout_prob=0.0,
                           drop_path_rate=0.0, layer_norm_eps=EPS)
