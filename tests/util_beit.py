"""float64 CPU restatements for the BEiT tests, written from the formulas of the operators' header
comments and torch's own operators (softmax, F.layer_norm, F.gelu, F.linear, F.conv2d, F.conv_transpose2d,
F.batch_norm, F.max_pool2d).  Token tensors are "rows x C" views [B, N, C] with head h in columns
[64 h, 64 h + 64), like the kernels' operands."""
import torch
import torch.nn.functional as F

from util_vit import HEAD_DIM, SCALE


def relpos_index(wh, ww):
    """[N, N] row of the bias table for (query i, key j), N = wh * ww + 1, written out pair by pair:
    token t >= 1 sits at divmod(t - 1, ww); R, R + 1, R + 2 are cls -> patch, patch -> cls, cls -> cls."""
    n, r = wh * ww + 1, (2 * wh - 1) * (2 * ww - 1)
    idx = torch.empty(n, n, dtype=torch.int64)
    for i in range(n):
        for j in range(n):
            if i == 0 and j == 0:
                idx[i, j] = r + 2
            elif i == 0:
                idx[i, j] = r
            elif j == 0:
                idx[i, j] = r + 1
            else:
                (iy, ix), (jy, jx) = divmod(i - 1, ww), divmod(j - 1, ww)
                idx[i, j] = (iy - jy + wh - 1) * (2 * ww - 1) + (ix - jx + ww - 1)
    return idx


def relpos_attention(q, k, v, heads, table, wh, ww, scale=SCALE):
    """softmax(scale * Q K^T + table[idx]) V per head in the dtype of the inputs -> (O [b, n, 64 heads],
    lse [b, heads, n]); ``table`` [(2 wh - 1)(2 ww - 1) + 3, >= heads] or None for no bias"""
    b, n, _ = q.shape
    qh, kh, vh = (t.view(b, n, heads, HEAD_DIM).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-2, -1)) * scale
    if table is not None:
        s = s + table[:, :heads].to(s.dtype)[relpos_index(wh, ww)].permute(2, 0, 1)
    o = s.softmax(dim=-1) @ vh
    return o.transpose(1, 2).reshape(b, n, heads * HEAD_DIM), torch.logsumexp(s, dim=-1)


# ---- the backbone ----------------------------------------------------------------------------------------
TINY = dict(embed_dim=128, num_heads=2, depth=4, out_indices=[0, 1, 2, 3], init_values=0.1, qkv_bias=True)
VARIANTS = {
    "p16-block-tables": dict(patch_size=16, img_size=(32, 48), use_rel_pos_bias=True, use_abs_pos_emb=False),
    "p16-shared-abs": dict(patch_size=16, img_size=(32, 48), use_shared_rel_pos_bias=True, use_abs_pos_emb=True),
    # patch 8 at 32 x 48 (window 4 x 6): the smallest image of this aspect whose stride-32 map exists -- at
    # 16 x 24 (window 2 x 3) fpn4's 4 / 4 max-pool has no output pixel at all
    "p8-block-tables": dict(patch_size=8, img_size=(32, 48), use_rel_pos_bias=True, use_abs_pos_emb=False),
}


def tiny_cfg(variant):
    return dict(type="BEiT", **{k: (list(v) if isinstance(v, list) else v) for k, v in TINY.items()},
                **VARIANTS[variant])


def randomize_beit(backbone, seed=0):
    """The constructor leaves the tables, q_bias / v_bias at zero, gamma at init_values and the BatchNorm
    at its identity statistics, which would hide every one of them: draw them all, and O(1) LayerNorm
    affines, tokens and weights that keep activations O(1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if "relative_position_bias_table" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 2.0)
            elif "gamma_" in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.4 + 0.1)
            elif ".norm" in name and name.endswith("weight") or name == "fpn1.1.weight":
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif name.startswith("fpn"):     # [Cin, Cout, 2, 2]
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[0] ** 0.5)
            elif p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
            elif name in ("cls_token", "pos_embed"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            else:
                raise AssertionError("unexpected parameter %s %s" % (name, tuple(p.shape)))
        for name, buf in backbone.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=g) * 0.3)
            elif name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=g) + 0.5)


def beit_ref(sd, x, cfg):
    """BEiT.forward on float64 tensors for a state dict ``sd`` and the constructor arguments ``cfg``: the four
    pyramid maps [B, D, H', W'] (strides 4, 8, 16, 32 of the image)."""
    d, heads, patch = cfg["embed_dim"], cfg["num_heads"], cfg["patch_size"]
    b = x.shape[0]
    wh, ww = x.shape[2] // patch, x.shape[3] // patch
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch)
    t = torch.cat([sd["cls_token"].expand(b, -1, -1), t.flatten(2).transpose(1, 2)], dim=1)
    if "pos_embed" in sd:
        t = t + sd["pos_embed"]
    shared = sd.get("rel_pos_bias.relative_position_bias_table")
    feats = []
    for i in range(cfg["depth"]):
        p = "blocks.%d." % i
        table = sd.get(p + "attn.relative_position_bias_table")
        if table is None:
            table = shared
        elif shared is not None:
            table = table + shared
        y = F.layer_norm(t, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        bias = None
        if p + "attn.q_bias" in sd:
            bias = torch.cat([sd[p + "attn.q_bias"], torch.zeros_like(sd[p + "attn.v_bias"]), sd[p + "attn.v_bias"]])
        q, k, v = F.linear(y, sd[p + "attn.qkv.weight"], bias).chunk(3, dim=-1)
        o, _ = relpos_attention(q.contiguous(), k.contiguous(), v.contiguous(), heads, table, wh, ww)
        o = F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        t = t + (sd[p + "gamma_1"] * o if p + "gamma_1" in sd else o)
        y = F.layer_norm(t, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])),
                     sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        t = t + (sd[p + "gamma_2"] * y if p + "gamma_2" in sd else y)
        if i in cfg["out_indices"]:
            feats.append(t[:, 1:].transpose(1, 2).reshape(b, d, wh, ww))

    def deconv(f, name):
        return F.conv_transpose2d(f, sd[name + ".weight"], sd[name + ".bias"], stride=2)

    if patch == 16:
        f = deconv(feats[0], "fpn1.0")
        f = F.batch_norm(f, sd["fpn1.1.running_mean"], sd["fpn1.1.running_var"], sd["fpn1.1.weight"],
                         sd["fpn1.1.bias"], False, 0.0, 1e-5)
        return [deconv(F.gelu(f), "fpn1.3"), deconv(feats[1], "fpn2.0"), feats[2], F.max_pool2d(feats[3], 2, 2)]
    return [deconv(feats[0], "fpn1.0"), feats[1], F.max_pool2d(feats[2], 2, 2), F.max_pool2d(feats[3], 4, 4)]


def double_sd(module):
    return {k: (v.detach().clone().double() if v.is_floating_point() else v.clone())
            for k, v in module.state_dict().items()}
