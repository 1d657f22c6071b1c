"""float64 CPU references for the ElasticConvformer coupling units and the whole backbone, written from the
maths and torch's own operators (F.conv2d, F.avg_pool2d, F.layer_norm, F.gelu, F.batch_norm, F.interpolate),
in the REFERENCE's operator order: the conv-to-token unit projects first and pools second, the kernels pool
first (the two commute in exact arithmetic, which the comparison therefore also checks)."""
import json
import os

import torch
import torch.nn.functional as F

from util_vit import attention_formula, ffn_width

LN_EPS = 1e-5     # what build_norm_layer gives a norm cfg without eps
BN_EPS = 1e-5


# ---- the two units -------------------------------------------------------------------------------------
def fcu_down_ref(z, x_t, weight, bias, eps):
    """z [B, T, D] (projected, pooled), x_t [B, T + 1, D] -> x_t + cat(x_t[:, :1], gelu(LN(z)))"""
    d = z.shape[-1]
    x = F.gelu(F.layer_norm(z, (d,), weight, bias, eps))
    return torch.cat([x_t[:, 0][:, None, :], x], dim=1) + x_t


def fcu_up_add_ref(x, r, s):
    """x [B, C, H, W] + F.interpolate(r [B, C, H / s, W / s], size=(H, W)) (nearest, torch's default)"""
    return x + F.interpolate(r, size=(r.shape[2] * s, r.shape[3] * s))


# ---- the backbone --------------------------------------------------------------------------------------
TINY = dict(embed_dim=128, num_heads=[2, 2, 2], mlp_ratio=[4, 4, 4], depth=9, stem_width=16,
            body_width=[32, 64, 128], body_depth=[2, 2, 2], patch_size=16)
H, W = 64, 96      # 24 tokens + cls, last map 2 x 3
SUBNETS = {"max": dict(stem=16, widths=[32, 64, 128], embed_dim=128, heads=[2, 2, 2], depths=[2, 2, 2],
                       ratios=[40, 40, 40]),
           "sub": dict(stem=16, widths=[16, 32, 64], embed_dim=64, heads=[1, 2, 1], depths=[1, 2, 1],
                       ratios=[30, 40, 35])}


def tiny_backbone_cfg(**kw):
    cfg = dict(type="ElasticConvformer", drop_path=0.0,
               **{k: (list(v) if isinstance(v, list) else v) for k, v in TINY.items()})
    cfg.update(kw)
    return cfg


def tiny_model_cfg(**kw):
    """DynamicUPerHead directly on the four maps of the tiny ElasticConvformer, FCN auxiliary head on stage 3"""
    from util_models import fcn_head, uper_head
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(**kw),
                decode_head=uper_head(in_channels=list(TINY["body_width"]) + [TINY["body_width"][2]], channels=16),
                auxiliary_head=fcn_head(in_channels=TINY["body_width"][2], in_index=2, channels=16, num_convs=1,
                                        concat_input=False, loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def nest(key, value):
    return {key: {key: value}}


def arch_of(name):
    """the arch of a subnet in the form ElasticConvformer.manipulate_arch takes"""
    a = SUBNETS[name]
    return {"stem": {"width": a["stem"]},
            "body": {"depth": list(a["depths"]),
                     "block": {"convblock": {"width": list(a["widths"])}, "embed_dim": {"width": a["embed_dim"]},
                               "transblock": {"MHA": nest("num_heads", list(a["heads"])),
                                              "FFN": nest("feedforward_channels", list(a["ratios"]))}}}}


def arch_meta(name):
    """the same as a flat sampler meta"""
    a = SUBNETS[name]
    blk = "arch.backbone.body.block."
    return {"name": name, "arch.backbone.stem.width": a["stem"], "arch.backbone.body.depth": list(a["depths"]),
            blk + "convblock.width": list(a["widths"]), blk + "embed_dim.width": a["embed_dim"],
            blk + "transblock.MHA.num_heads.num_heads": list(a["heads"]),
            blk + "transblock.FFN.feedforward_channels.feedforward_channels": list(a["ratios"])}


SEED, IMG_SEED = 0, 1     # of the parameters and of the image the gradient-parity test uses
MARGIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convformer_relu_margin.json")


def randomize_convformer(backbone, seed=SEED, margin=True):
    """O(1) norm affines, tokens and biases, weights that keep activations O(1), running statistics that are
    not the identity.  ``margin`` (with the seed of record): the BatchNorm biases that
    tests/golden/make_convformer_relu_margin.py moved are set to their recorded values, which keeps every
    ReLU input of the float64 model at least 1e-4 rms away from zero for image seed IMG_SEED."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            leaf = name.rsplit(".", 2)[-2] if "." in name else name
            if leaf.startswith("bn") and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
            elif leaf.startswith("bn"):
                w = dict(backbone.named_parameters())[name[:-4] + "weight"]
                p.copy_(w * (torch.rand(p.shape, generator=g) + 1.5))
            elif leaf.startswith("ln") and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
            elif "embeddings_table" in name or name == "cls_token":
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            else:
                raise AssertionError("unexpected parameter %s %s" % (name, tuple(p.shape)))
        for name, b in backbone.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
        if margin and seed == SEED:
            with open(MARGIN_FILE) as f:
                moved = json.load(f)["bias"]
            params = dict(backbone.named_parameters())
            for name, values in moved.items():
                for c, value in values:
                    params[name][c] = float(value)


def convformer_ref(sd, img, arch, norm_eval=True, patch=16, relu_inputs=None):
    """The ElasticConvformer in training mode on float64 tensors, for a state dict of max-size tensors ``sd``
    (2-D linear weights) and the subnet ``arch`` (an entry of SUBNETS): leading slices of every parameter,
    the first depths[i] blocks of stage i.  The stem's BatchNorm always uses its running statistics (it is
    frozen), the others do with ``norm_eval``.  Returns the four feature maps; every ReLU's input is appended
    to ``relu_inputs`` when that is a list, as (name of the BatchNorm bias that shifts it, tensor)."""
    d = arch["embed_dim"]
    b = img.shape[0]

    def relu(v, name):
        if relu_inputs is not None:
            relu_inputs.append((name + ".bias", v))
        return F.relu(v)

    def conv(v, name, co, stride=1, pad=0):
        bias = sd.get(name + ".bias")
        return F.conv2d(v, sd[name + ".weight"][:co, :v.shape[1]], None if bias is None else bias[:co],
                        stride=stride, padding=pad)

    def bn(v, name, frozen=False):
        c = v.shape[1]
        wt, bs = sd[name + ".weight"][:c], sd[name + ".bias"][:c]
        if frozen or norm_eval:
            return F.batch_norm(v, sd[name + ".running_mean"][:c].detach(), sd[name + ".running_var"][:c].detach(),
                                wt, bs, False, 0., BN_EPS)
        return F.batch_norm(v, None, None, wt, bs, True, 0., BN_EPS)

    def lin(v, name, co):
        return F.linear(v, sd[name + ".weight"][:co, :v.shape[-1]], sd[name + ".bias"][:co])

    def ln(v, name):
        return F.layer_norm(v, (d,), sd[name + ".weight"][:d], sd[name + ".bias"][:d], LN_EPS)

    def conv_block(v, p, width, stride=1, res_conv=False, x_t=None, s=1):
        med = width // 4
        y = relu(bn(conv(v, p + "conv1", med), p + "bn1"), p + "bn1")
        if x_t is not None:
            y = fcu_up_add_ref(y, x_t, s)
        x2 = relu(bn(conv(y, p + "conv2", med, stride, 1), p + "bn2"), p + "bn2")
        y = bn(conv(x2, p + "conv3", width), p + "bn3")
        res = bn(conv(v, p + "residual_conv", width, stride), p + "bn4") if res_conv else v
        return relu(y + res, p + "bn3"), x2

    def trans_block(t, p, heads, ratio):
        y = ln(t, p + "ln1")
        o, _ = attention_formula(lin(y, p + "attn.w_qs", 64 * heads), lin(y, p + "attn.w_ks", 64 * heads),
                                 lin(y, p + "attn.w_vs", 64 * heads), heads)
        t = t + lin(o, p + "attn.proj", d)
        return t + lin(F.gelu(lin(ln(t, p + "ln2"), p + "mlp.layer1", ffn_width(ratio, d))), p + "mlp.layer2", d)

    x = F.max_pool2d(relu(bn(conv(img, "conv1", arch["stem"], 2, 3), "bn1", frozen=True), "bn1"), 3, 2, 1)
    strides = [patch // 4, patch // 8, patch // 16, patch // 16]
    outs, x_t = [], None
    for i in range(4):
        j = min(i, 2)
        width, heads, ratio, s = arch["widths"][j], arch["heads"][j], arch["ratios"][j], strides[i]
        for k in range(arch["depths"][i] if i < 3 else 1):
            p = "conv_trans_%d.%d." % (i + 1, k)
            if i == 0 and k == 0:
                x_base = x
                x, _ = conv_block(x_base, p + "conv_1.", width, res_conv=True)
                t = conv(x_base, p + "trans_patch_conv", d, s).flatten(2).transpose(1, 2)
                x_t = trans_block(torch.cat([sd["cls_token"][:, :, :d].expand(b, -1, -1), t], dim=1),
                                  p + "trans_1.", heads, ratio)
                continue
            x, x2 = conv_block(x, p + "cnn_block.", width, stride=2 if (i in (1, 2) and k == 0) else 1,
                               res_conv=k == 0 and i != 3)
            hh, ww = x2.shape[2] // s, x2.shape[3] // s
            z = F.avg_pool2d(conv(x2, p + "squeeze_block.conv_project", d), s, s).flatten(2).transpose(1, 2)
            q = p + "squeeze_block.ln1"
            x_t = trans_block(fcu_down_ref(z, x_t, sd[q + ".weight"][:d], sd[q + ".bias"][:d], LN_EPS),
                              p + "trans_block.", heads, ratio)
            x_r = x_t[:, 1:].transpose(1, 2).reshape(b, d, hh, ww)
            x_r = relu(bn(conv(x_r, p + "expand_block.conv_project", width // 4), p + "expand_block.bn1"),
                       p + "expand_block.bn1")
            x, _ = conv_block(x, p + "fusion_block.", width, stride=2 if i == 3 else 1, res_conv=i == 3, x_t=x_r,
                              s=s)
        outs.append(x)
    return outs


RELU_MARGIN = 1e-4


def assert_relu_margin(relu_inputs):
    """no ReLU input (as convformer_ref collects them) lies within RELU_MARGIN rms of zero"""
    worst = min((float(v.detach().abs().min() / v.detach().pow(2).mean().sqrt()), name) for name, v in relu_inputs)
    print("smallest |ReLU input| / rms: %.3g (%s)" % worst)
    assert worst[0] >= RELU_MARGIN, "a ReLU input within %g rms of zero behind %s: %.3g" % (
        RELU_MARGIN, worst[1], worst[0])


def active_slice(name, arch):
    """index of the part of state-dict tensor ``name`` that subnet ``arch`` reads, or None where it reads
    nothing of it (a skipped block, the relative-position tables)"""
    d = arch["embed_dim"]
    if name == "cls_token":
        return (slice(None), slice(None), slice(0, d))
    if name.startswith(("conv1.", "bn1.")):
        return (slice(0, arch["stem"]),)
    if "rel_pos_embed" in name:
        return None
    stage, block, rest = name[len("conv_trans_"):].split(".", 2)
    i, k = int(stage) - 1, int(block)
    j = min(i, 2)
    if k >= (arch["depths"][i] if i < 3 else 1):
        return None
    width, hw, hidden = arch["widths"][j], 64 * arch["heads"][j], ffn_width(arch["ratios"][j], d)
    med = width // 4
    prev = arch["stem"] if i == 0 else arch["widths"][min(i - 1, 2)]
    unit, rest = rest.split(".", 1)
    mod, kind = rest.rsplit(".", 1) if "." in rest else ("", rest)
    if unit in ("conv_1", "cnn_block", "fusion_block"):
        cin = width if (unit == "fusion_block" or k > 0 or i == 3) else prev
        out, inp = {"conv1": (med, cin), "bn1": (med, None), "conv2": (med, med), "bn2": (med, None),
                    "conv3": (width, med), "bn3": (width, None), "residual_conv": (width, cin),
                    "bn4": (width, None)}[mod]
    elif unit == "trans_patch_conv":
        out, inp = d, prev
    elif unit == "squeeze_block":
        out, inp = {"conv_project": (d, med), "ln1": (d, None)}[mod]
    elif unit == "expand_block":
        out, inp = {"conv_project": (med, d), "bn1": (med, None)}[mod]
    else:
        out, inp = {"ln1": (d, None), "ln2": (d, None), "attn.w_qs": (hw, d), "attn.w_ks": (hw, d),
                    "attn.w_vs": (hw, d), "attn.proj": (d, hw), "mlp.layer1": (hidden, d),
                    "mlp.layer2": (d, hidden)}[mod]
    return (slice(0, out), slice(0, inp)) if kind == "weight" and inp is not None else (slice(0, out),)
