"""Plain torch restatements of SegNeXt's MSCAN encoder (mmseg's ``mscan.py``), written from the network's
definition with torch's own operators: ``mscan_ref`` on a state dict in the dtype of the image (float64: the
reference), and ``PlainMSCAN``, the same network as stock nn.Conv2d / nn.BatchNorm2d / nn.LayerNorm modules
under mmseg's names, whose state dict a DynamicMSCAN of that size must load strictly."""
import torch
import torch.nn as nn
import torch.nn.functional as F

KERNELS = (7, 11, 21)
# supernet maxima of the tiny backbone and the subnet the tests cut out of it
TINY = dict(embed_dims=[16, 24, 32, 40], depths=[2, 1, 2, 1], mlp_ratios=[4, 4, 2, 2])
SUBNETS = {"max": dict(depth=[2, 1, 2, 1], width=[16, 24, 32, 40], mlp_ratio=[4, 4, 2, 2]),
           "sub": dict(depth=[1, 1, 1, 1], width=[8, 16, 24, 32], mlp_ratio=[2, 4, 2, 1])}
BN_EPS, LN_EPS = 1e-5, 1e-5


def tiny_backbone_cfg(**kw):
    cfg = dict(type="DynamicMSCAN", norm_cfg=dict(type="SyncBN", requires_grad=True),
               **{k: list(v) for k, v in TINY.items()})
    cfg.update(kw)
    return cfg


def tiny_model_cfg():
    """DynamicUPerHead on the four maps of the tiny DynamicMSCAN, FCN auxiliary head on stage 3"""
    from util_models import fcn_head, uper_head
    w = TINY["embed_dims"]
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(), decode_head=uper_head(w, channels=16),
                auxiliary_head=fcn_head(in_channels=w[2], in_index=2, channels=16, num_convs=1, concat_input=False,
                                        loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def arch_of(name):
    """the arch of a subnet in the form DynamicMSCAN.manipulate_arch takes"""
    return {"body": {k: list(v) for k, v in SUBNETS[name].items()}}


def arch_meta(name):
    """the same as a flat sampler meta"""
    return dict({"name": name}, **{"arch.backbone.body." + k: list(v) for k, v in SUBNETS[name].items()})


def hidden_width(ratio, c):
    return int(ratio * c)


def randomize_mscan(backbone, seed=0):
    """O(1) norm weights and running variances, small biases and running means, layer scales of O(1) (at
    their initial 1e-2 an error inside a branch would hide below the tolerance), weights that keep
    activations O(1)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if "layer_scale" in name:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
            elif p.dim() == 1 and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
        for name, b in backbone.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def mscan_ref(sd, img, arch, training=True):
    """MSCAN on the tensors of ``sd`` (max-size tensors under mmseg's names) in the dtype of ``img`` for the
    subnet ``arch`` (an entry of SUBNETS): leading slices of every parameter, the first depth[i] blocks of
    stage i.  BatchNorm on batch statistics (``training``) or on the running ones.  Returns the four feature
    maps [B, C_i, H_i, W_i]."""
    def conv(x, name, co, **kw):
        return F.conv2d(x, sd[name + ".weight"][:co, :x.shape[1]], sd[name + ".bias"][:co], **kw)

    def dw(x, name, padding):
        c = x.shape[1]
        return F.conv2d(x, sd[name + ".weight"][:c], sd[name + ".bias"][:c], padding=padding, groups=c)

    def bn(x, name):
        c = x.shape[1]
        if training:
            return F.batch_norm(x, None, None, sd[name + ".weight"][:c], sd[name + ".bias"][:c], True, 0.0, BN_EPS)
        return F.batch_norm(x, sd[name + ".running_mean"][:c], sd[name + ".running_var"][:c],
                            sd[name + ".weight"][:c], sd[name + ".bias"][:c], False, 0.0, BN_EPS)

    outs, x = [], img
    for i in range(4):
        c, depth = arch["width"][i], arch["depth"][i]
        hidden = hidden_width(arch["mlp_ratio"][i], c)
        pe = "patch_embed%d." % (i + 1)
        if i == 0:
            x = F.gelu(bn(conv(x, pe + "proj.0", c // 2, stride=2, padding=1), pe + "proj.1"))
            x = bn(conv(x, pe + "proj.3", c, stride=2, padding=1), pe + "proj.4")
        else:
            x = bn(conv(x, pe + "proj", c, stride=2, padding=1), pe + "norm")
        for j in range(depth):
            q = "block%d.%d." % (i + 1, j)
            sgu = q + "attn.spatial_gating_unit."
            n1 = bn(x, q + "norm1")
            u = F.gelu(conv(n1, q + "attn.proj_1", c))
            a = dw(u, sgu + "conv0", 2)
            s = a
            for b, k in enumerate(KERNELS):
                s = s + dw(dw(a, sgu + "conv%d_1" % b, (0, k // 2)), sgu + "conv%d_2" % b, (k // 2, 0))
            g = conv(s, sgu + "conv3", c) * u
            x = x + sd[q + "layer_scale_1"][:c].view(1, c, 1, 1) * (conv(g, q + "attn.proj_2", c) + n1)
            z = dw(conv(bn(x, q + "norm2"), q + "mlp.fc1", hidden), q + "mlp.dwconv", 1)
            x = x + sd[q + "layer_scale_2"][:c].view(1, c, 1, 1) * conv(F.gelu(z), q + "mlp.fc2", c)
        nm = "norm%d" % (i + 1)
        x = F.layer_norm(x.permute(0, 2, 3, 1), (c,), sd[nm + ".weight"][:c], sd[nm + ".bias"][:c], LN_EPS)
        x = x.permute(0, 3, 1, 2).contiguous()
        outs.append(x)
    return outs


def active_slice(name, arch):
    """index of the part of state-dict tensor ``name`` that subnet ``arch`` reads, or None where it reads
    nothing of it (a block past the stage's depth)"""
    parts = name.split(".")
    i = int(parts[0][-1]) - 1
    c = arch["width"][i]
    c_in = 3 if i == 0 else arch["width"][i - 1]
    hidden = hidden_width(arch["mlp_ratio"][i], c)
    kind = parts[-1]
    if parts[0].startswith("norm"):
        return (slice(0, c),)
    if parts[0].startswith("patch_embed"):
        if i == 0:
            co, ci = {"0": (c // 2, 3), "1": (c // 2, None), "3": (c, c // 2), "4": (c, None)}[parts[2]]
        else:
            co, ci = (c, c_in) if parts[1] == "proj" else (c, None)
        return (slice(0, co), slice(0, ci)) if kind == "weight" and ci is not None else (slice(0, co),)
    if int(parts[1]) >= arch["depth"][i]:
        return None
    mod = ".".join(parts[2:-1]) if len(parts) > 3 else parts[2]
    if mod in ("mlp.fc1", "mlp.fc2", "attn.proj_1", "attn.proj_2", "attn.spatial_gating_unit.conv3"):
        co, ci = {"mlp.fc1": (hidden, c), "mlp.fc2": (c, hidden)}.get(mod, (c, c))
        return (slice(0, co), slice(0, ci)) if kind == "weight" else (slice(0, co),)
    return (slice(0, hidden if mod == "mlp.dwconv" else c),)


def param_count(arch):
    """parameters of a standalone MSCAN of the sizes of ``arch``"""
    total, ci = 0, 3
    for i in range(4):
        c, hidden = arch["width"][i], hidden_width(arch["mlp_ratio"][i], arch["width"][i])
        if i == 0:
            total += (c // 2) * 3 * 9 + c // 2 + 2 * (c // 2) + c * (c // 2) * 9 + c + 2 * c
        else:
            total += c * ci * 9 + c + 2 * c
        block = 2 * 2 * c + 2 * c                                   # norm1, norm2, layer scales
        block += 3 * (c * c + c)                                    # proj_1, conv3, proj_2
        block += 25 * c + c + sum(2 * (k * c + c) for k in KERNELS)  # the depthwise filters
        block += hidden * c + hidden + 9 * hidden + hidden + c * hidden + c
        total += arch["depth"][i] * block + 2 * c                   # + norm{i}
        ci = c
    return total


# ---- the same network as stock modules under mmseg's names ---------------------------------------------
class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv0 = nn.Conv2d(c, c, 5, padding=2, groups=c)
        for b, k in enumerate(KERNELS):
            setattr(self, "conv%d_1" % b, nn.Conv2d(c, c, (1, k), padding=(0, k // 2), groups=c))
            setattr(self, "conv%d_2" % b, nn.Conv2d(c, c, (k, 1), padding=(k // 2, 0), groups=c))
        self.conv3 = nn.Conv2d(c, c, 1)

    def forward(self, u):
        a = self.conv0(u)
        s = a
        for b in range(3):
            s = s + getattr(self, "conv%d_2" % b)(getattr(self, "conv%d_1" % b)(a))
        return self.conv3(s) * u


class _SpatialAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.proj_1 = nn.Conv2d(c, c, 1)
        self.activation = nn.GELU()
        self.spatial_gating_unit = _Attention(c)
        self.proj_2 = nn.Conv2d(c, c, 1)

    def forward(self, n1):
        return self.proj_2(self.spatial_gating_unit(self.activation(self.proj_1(n1)))) + n1


class _Mlp(nn.Module):
    def __init__(self, c, hidden):
        super().__init__()
        self.fc1 = nn.Conv2d(c, hidden, 1)
        self.dwconv = nn.Conv2d(hidden, hidden, 3, padding=1, groups=hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Conv2d(hidden, c, 1)

    def forward(self, x):
        return self.fc2(self.act(self.dwconv(self.fc1(x))))


class _Block(nn.Module):
    def __init__(self, c, hidden):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(c)
        self.attn = _SpatialAttention(c)
        self.norm2 = nn.BatchNorm2d(c)
        self.mlp = _Mlp(c, hidden)
        self.layer_scale_1 = nn.Parameter(1e-2 * torch.ones(c))
        self.layer_scale_2 = nn.Parameter(1e-2 * torch.ones(c))

    def forward(self, x):
        x = x + self.layer_scale_1.view(1, -1, 1, 1) * self.attn(self.norm1(x))
        return x + self.layer_scale_2.view(1, -1, 1, 1) * self.mlp(self.norm2(x))


class _Stem(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(3, c // 2, 3, 2, 1), nn.BatchNorm2d(c // 2), nn.GELU(),
                                  nn.Conv2d(c // 2, c, 3, 2, 1), nn.BatchNorm2d(c))

    def forward(self, x):
        return self.proj(x)


class _PatchEmbed(nn.Module):
    def __init__(self, ci, c):
        super().__init__()
        self.proj = nn.Conv2d(ci, c, 3, 2, 1)
        self.norm = nn.BatchNorm2d(c)

    def forward(self, x):
        return self.norm(self.proj(x))


class PlainMSCAN(nn.Module):
    """a standalone MSCAN of the sizes of ``arch`` (an entry of SUBNETS)"""

    def __init__(self, arch):
        super().__init__()
        ci = 3
        for i in range(4):
            c = arch["width"][i]
            setattr(self, "patch_embed%d" % (i + 1), _Stem(c) if i == 0 else _PatchEmbed(ci, c))
            setattr(self, "block%d" % (i + 1), nn.ModuleList(
                [_Block(c, hidden_width(arch["mlp_ratio"][i], c)) for _ in range(arch["depth"][i])]))
            setattr(self, "norm%d" % (i + 1), nn.LayerNorm(c, eps=LN_EPS))
            ci = c

    def forward(self, x):
        outs = []
        for i in range(4):
            x = getattr(self, "patch_embed%d" % (i + 1))(x)
            for block in getattr(self, "block%d" % (i + 1)):
                x = block(x)
            x = getattr(self, "norm%d" % (i + 1))(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).contiguous()
            outs.append(x)
        return outs
