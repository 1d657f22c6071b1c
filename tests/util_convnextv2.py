"""float64 CPU references for ConvNeXt V2: the GELU + GRN operator and the backbone, written from the
maths and torch's own operators (not from transformers, which tests/test_convnextv2.py compares them
with), on leading slices of a state dict with transformers' ``ConvNextV2Backbone`` names."""
import torch
import torch.nn.functional as F

# the tiny supernet of the ConvNeXt tests
TINY = dict(dims=(8, 16, 24, 32), depths=(2, 2, 3, 2))
SUBNETS = {"max": dict(width=[8, 16, 24, 32], depth=[2, 2, 3, 2]),
           "sub": dict(width=[4, 8, 12, 16], depth=[1, 2, 2, 1])}
STAGES = ["stage1", "stage2", "stage3", "stage4"]


# ---- the operator --------------------------------------------------------------------------------------
def grn_formula(a, weight, bias, eps=1e-6):
    """GRN of a [N, H, W, C] (or [N, P, C]) tensor with [C] parameters: G the 2-norm over the pixels of a
    sample, Nx = G / (mean_c G + eps), y = a * (1 + weight * Nx) + bias"""
    dims = tuple(range(1, a.dim() - 1))
    # torch's 2-norm: its gradient at a zero vector is zero (sum(a^2).sqrt() would give 0 * inf = NaN there)
    g = torch.linalg.vector_norm(a, ord=2, dim=dims, keepdim=True)
    nx = g / (g.mean(-1, keepdim=True) + eps)
    return a * (1 + weight * nx) + bias


def gelu_grn_ref(x, weight, bias, dy, eps=1e-6):
    """x, dy [N, P, C]; weight, bias [C] -> (y, G [N, C], dx, dweight, dbias) in float64 by autograd"""
    xr = x.double().requires_grad_(True)
    wr, br = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    a = F.gelu(xr)
    y = grn_formula(a, wr, br, eps)
    y.backward(dy.double())
    return y.detach(), a.detach().pow(2).sum(1).sqrt(), xr.grad, wr.grad, br.grad


# ---- the backbone --------------------------------------------------------------------------------------
def tiny_backbone_cfg(**kw):
    cfg = dict(type="DynamicConvNeXtV2", depths=list(TINY["depths"]), dims=list(TINY["dims"]), drop_path_rate=0.0,
               out_indices=[0, 1, 2, 3])
    cfg.update(kw)
    return cfg


def tiny_model_cfg():
    """DynamicUPerHead on the tiny ConvNeXt V2 supernet, with the FCN auxiliary head on stage 3"""
    from util_models import fcn_head, uper_head
    return dict(type="DynamicEncoderDecoder", backbone=tiny_backbone_cfg(),
                decode_head=uper_head(in_channels=TINY["dims"], channels=16),
                auxiliary_head=fcn_head(in_channels=TINY["dims"][2], in_index=2, channels=16, num_convs=1,
                                        concat_input=False, loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def arch_meta(name):
    a = SUBNETS[name]
    return {"name": name, "arch.backbone.body.width": list(a["width"]), "arch.backbone.body.depth": list(a["depth"])}


def hf_config(arch):
    """transformers' config of a fixed ConvNeXt V2 backbone of exactly the sizes of ``arch``"""
    import transformers
    return transformers.ConvNextV2Config(hidden_sizes=list(arch["width"]), depths=list(arch["depth"]),
                                         out_features=list(STAGES))


def randomize_convnextv2(backbone, seed=0):
    """O(1) GRN weights and biases and LayerNorm affines (at the zero init GRN is the identity and no test
    would see it), conv / linear weights of a size that keeps activations O(1), nonzero biases"""
    from gaia_seg_amd.core.bricks import DynamicConv2d, DynamicGRN, DynamicLayerNorm
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in backbone.modules():
            if isinstance(m, DynamicGRN):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            elif isinstance(m, DynamicLayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            elif isinstance(m, DynamicConv2d):
                p = m.weight
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)


def convnextv2_ref(sd, x, width, depth, out_indices=(0, 1, 2, 3), eps=1e-6):
    """The ConvNeXt V2 backbone on float64 NCHW tensors from torch's own operators, for a state dict of
    max-size tensors ``sd`` (transformers' names, 2-D linear weights, [1, 1, 1, 4C] GRN parameters) and the
    subnet (width, depth): leading slices of every parameter, the first depth[i] blocks of stage i.
    Returns the normalised output features."""
    def ln(t, name, c):     # LayerNorm over the channels of an NCHW tensor
        return F.layer_norm(t.permute(0, 2, 3, 1), (c,), sd[name + ".weight"][:c], sd[name + ".bias"][:c],
                            eps).permute(0, 3, 1, 2)

    c = width[0]
    t = F.conv2d(x, sd["embeddings.patch_embeddings.weight"][:c], sd["embeddings.patch_embeddings.bias"][:c], stride=4)
    t = ln(t, "embeddings.layernorm", c)
    outs = []
    for i in range(4):
        s = "encoder.stages.%d." % i
        if i:
            cn = width[i]
            t = F.conv2d(ln(t, s + "downsampling_layer.0", c), sd[s + "downsampling_layer.1.weight"][:cn, :c],
                         sd[s + "downsampling_layer.1.bias"][:cn], stride=2)
            c = cn
        for j in range(depth[i]):
            p = s + "layers.%d." % j
            y = F.conv2d(t, sd[p + "dwconv.weight"][:c], sd[p + "dwconv.bias"][:c], padding=3, groups=c)
            y = F.layer_norm(y.permute(0, 2, 3, 1), (c,), sd[p + "layernorm.weight"][:c], sd[p + "layernorm.bias"][:c],
                             eps)
            y = F.gelu(F.linear(y, sd[p + "pwconv1.weight"][:4 * c, :c], sd[p + "pwconv1.bias"][:4 * c]))
            y = grn_formula(y, sd[p + "grn.weight"][0, 0, 0, :4 * c], sd[p + "grn.bias"][0, 0, 0, :4 * c])
            y = F.linear(y, sd[p + "pwconv2.weight"][:c, :4 * c], sd[p + "pwconv2.bias"][:c])
            t = t + y.permute(0, 3, 1, 2)
        if i in out_indices:
            outs.append(ln(t, "hidden_states_norms.stage%d" % (i + 1), c))
    return outs


def slice_state_dict(sd, shapes):
    """the leading slices of the max-size state dict ``sd`` that a fixed network holds: ``shapes`` is that
    network's own {name: shape} (its blocks beyond the subnet's depths have no names there)"""
    return {k: sd[k][tuple(slice(0, n) for n in shp)].clone() for k, shp in shapes.items()}


def convnextv2_param_count(dims, depths, in_chans=3):
    """closed form: parameters of a ConvNeXt V2 backbone (stem, downsample layers, blocks with the GRN weight
    and bias of the 4C-wide hidden layer in place of V1's layer scale, the four output norms)"""
    n = in_chans * dims[0] * 16 + dims[0] + 2 * dims[0]                       # stem conv + LN
    for i in range(1, 4):
        n += 2 * dims[i - 1] + dims[i - 1] * dims[i] * 4 + dims[i]           # LN + 2x2 conv
    for d, k in zip(dims, depths):
        n += k * ((49 * d + d) + 2 * d + (4 * d * d + 4 * d) + (4 * d * d + d) + 2 * 4 * d)   # dw, LN, pw1, pw2, GRN
    return n + sum(2 * d for d in dims)                                       # the four output norms
