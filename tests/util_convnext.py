"""float64 CPU references for the ConvNeXt operators and backbone, written from the maths and from
torch's own modules (F.conv2d(groups=C), F.layer_norm, F.gelu, nn.Linear).  Everything is NHWC
("rows x C" for the pointwise operators), like the kernels' operands."""
import torch
import torch.nn.functional as F


def dwconv_ref(x, w, dy, pad, dil):
    """x [n,h,w,c], w [k,k,c], dy [n,ho,wo,c] -> (y, dx, dw) in the same layouts, float64"""
    c = x.shape[-1]
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().permute(2, 0, 1).unsqueeze(1).requires_grad_(True)          # [c, 1, k, k]
    y = F.conv2d(xr, wr, None, 1, pad, dil, groups=c)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous(),
            wr.grad.squeeze(1).permute(1, 2, 0).contiguous())


def layernorm_ref(x, weight, bias, dy, eps):
    """x, dy [rows, c] -> (y, mean, rstd, dx, dweight, dbias), float64"""
    xr = x.double().requires_grad_(True)
    wr, br = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[-1],), wr, br, eps)
    y.backward(dy.double())
    mean = xr.detach().mean(-1)
    rstd = (xr.detach().var(-1, unbiased=False) + eps).rsqrt()
    return y.detach(), mean, rstd, xr.grad, wr.grad, br.grad


def gelu_ref(x, dy):
    xr = x.double().requires_grad_(True)
    y = F.gelu(xr)
    y.backward(dy.double())
    return y.detach(), xr.grad


def layer_scale_ref(identity, z, gamma, dout):
    """out = identity + gamma * z; -> (out, dz, dgamma), float64"""
    zr, gr = z.double().requires_grad_(True), gamma.double().requires_grad_(True)
    out = identity.double() + gr * zr
    out.backward(dout.double())
    return out.detach(), zr.grad, gr.grad


# ---- the backbone ------------------------------------------------------------------------------------
TINY = dict(dims=(8, 16, 24, 32), depths=(2, 2, 3, 2))
SUBNETS = {"max": dict(width=[8, 16, 24, 32], depth=[2, 2, 3, 2]),
           "sub": dict(width=[4, 8, 12, 16], depth=[1, 2, 2, 1])}


def tiny_backbone_cfg(**kw):
    cfg = dict(type="DynamicConvNeXt", depths=list(TINY["depths"]), dims=list(TINY["dims"]), drop_path_rate=0.0,
               out_indices=[0, 1, 2, 3], layer_scale_init_value=1e-6, conv_cfg=dict(type="DynConv2d"))
    cfg.update(kw)
    return cfg


def tiny_model_cfg():
    """DynamicUPerHead on the tiny ConvNeXt supernet, with the FCN auxiliary head on stage 3"""
    from util_models import fcn_head, uper_head
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(),
                decode_head=uper_head(in_channels=TINY["dims"], channels=16),
                auxiliary_head=fcn_head(in_channels=TINY["dims"][2], in_index=2, channels=16, num_convs=1,
                                        concat_input=False, loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def arch_meta(name):
    a = SUBNETS[name]
    return {"name": name, "arch.backbone.body.width": list(a["width"]), "arch.backbone.body.depth": list(a["depth"])}


def randomize_convnext(backbone, seed=0):
    """O(1) layer scales and LayerNorm affines (at the 1e-6 gamma init the residual branch is invisible
    to any tolerance), conv / linear weights of a size that keeps activations O(1), nonzero biases"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if name.endswith("gamma"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1 and (".ln" in "." + name or name.startswith("norm") or name.startswith("ln")) \
                    and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                fan_in = p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g) / fan_in ** 0.5)


def convnext_ref(sd, x, width, depth, out_indices=(0, 1, 2, 3), eps=1e-6):
    """The ConvNeXt backbone on float64 NCHW tensors from torch's own operators, for a state dict of
    max-size tensors ``sd`` (2-D linear weights) and the subnet (width, depth): leading slices of every
    parameter, the first depth[i] blocks of stage i.  Returns the normalised output features."""
    def ln(t, name, c):     # LayerNorm over the channels of an NCHW tensor
        return F.layer_norm(t.permute(0, 2, 3, 1), (c,), sd[name + ".weight"][:c], sd[name + ".bias"][:c],
                            eps).permute(0, 3, 1, 2)

    c = width[0]
    t = ln(F.conv2d(x, sd["stem.weight"][:c], sd["stem.bias"][:c], stride=4), "ln1", c)
    outs = []
    for i in range(4):
        c = width[i]
        for j in range(depth[i]):
            p = "dynamic_convnext_block_%d.%d." % (i + 1, j)
            y = F.conv2d(t, sd[p + "dwconv.weight"][:c], sd[p + "dwconv.bias"][:c], padding=3, groups=c)
            y = F.layer_norm(y.permute(0, 2, 3, 1), (c,), sd[p + "ln1.weight"][:c], sd[p + "ln1.bias"][:c], eps)
            y = F.gelu(F.linear(y, sd[p + "pwconv1.weight"][:4 * c, :c], sd[p + "pwconv1.bias"][:4 * c]))
            y = F.linear(y, sd[p + "pwconv2.weight"][:c, :4 * c], sd[p + "pwconv2.bias"][:c])
            if p + "gamma" in sd:
                y = sd[p + "gamma"][:c] * y
            t = t + y.permute(0, 3, 1, 2)
        if i in out_indices:
            outs.append(ln(t, "norm%d" % i, c))
        if i < 3:
            cn = width[i + 1]
            t = F.conv2d(ln(t, "ln%d" % (i + 2), c), sd["ds%d_conv.weight" % (i + 1)][:cn, :c],
                         sd["ds%d_conv.bias" % (i + 1)][:cn], stride=2)
    return outs


def convnext_param_count(dims, depths, in_chans=3):
    """closed form: parameters of a ConvNeXt backbone (stem, downsample layers, blocks with layer scale,
    the four output norms)"""
    n = in_chans * dims[0] * 16 + dims[0] + 2 * dims[0]                       # stem conv + LN
    for i in range(1, 4):
        n += 2 * dims[i - 1] + dims[i - 1] * dims[i] * 4 + dims[i]           # LN + 2x2 conv
    for d, k in zip(dims, depths):
        block = (49 * d + d) + 2 * d + (4 * d * d + 4 * d) + (4 * d * d + d) + d   # dw, LN, pw1, pw2, gamma
        n += k * block
    return n + sum(2 * d for d in dims)                                       # norm0..3
