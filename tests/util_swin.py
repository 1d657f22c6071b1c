"""What the Swin tests share: the float64 restatement of gs_window_attention_* (transformers' SwinLayer with
always_partition: roll, window partition, relative-position bias, region mask, softmax, reverse, roll back) in
plain torch through autograd, the 2x2-cell LayerNorm of the patch merging, and the operator cases."""
import torch

HEAD_DIM = 32
SCALE = HEAD_DIM ** -0.5

# (name, B, H, W, ws, shift, heads, sliced operands + wide ldo + ld_table 5?, dominant?)
WA_CASES = [
    ("one", 1, 7, 7, 7, 0, 1, False, False),
    ("shift", 2, 14, 21, 7, 3, 3, True, False),
    ("wrapH", 1, 7, 14, 7, 3, 2, False, False),
    ("ws8", 2, 16, 8, 8, 4, 2, False, False),
    ("ws4", 1, 8, 12, 4, 2, 5, False, False),
    ("ws2", 1, 4, 6, 2, 1, 1, False, False),
    ("dominant", 2, 14, 14, 7, 3, 2, False, True),
]
SPLIT_CASE = (2, 28, 35, 7, 3, 2)   # 40 windows
SPLITS = (1, 2, 3, 40)


def table_rows(ws):
    return (2 * ws - 1) ** 2


def wa_geometry(h, w, ws, shift):
    """-> (pix [windows, ws^2]: the pixel y * W + x of every window token, idx [ws^2, ws^2]: the table row of a
    pair, mask [windows, ws^2, ws^2] of 0 / -100 or None without a shift)"""
    yp, xp = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")   # the shifted frame
    pix = ((yp + shift) % h) * w + (xp + shift) % w

    def windows(t):
        return t.view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)

    iy, ix = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    iy, ix = iy.reshape(-1), ix.reshape(-1)
    idx = (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)
    mask = None
    if shift > 0:
        def r(t, n):
            return (t >= n - ws).long() + (t >= n - shift).long()
        region = windows(3 * r(yp, h) + r(xp, w))
        mask = torch.where(region[:, :, None] == region[:, None, :], 0.0, -100.0)
    return windows(pix), idx, mask


def wa_formula(q, k, v, table, b, h, w, ws, shift, heads):
    """q, k, v [B, H*W, 32 heads], table [(2 ws - 1)^2, >= heads] -> (O [B, H*W, 32 heads], lse [B, heads, H*W])"""
    pix, idx, mask = wa_geometry(h, w, ws, shift)
    nw, n = pix.shape
    flat = pix.reshape(-1)
    inv = torch.argsort(flat)

    def part(t):
        return t[:, flat].view(b, nw, n, heads, HEAD_DIM).permute(0, 1, 3, 2, 4)

    s = SCALE * (part(q) @ part(k).transpose(-1, -2))
    s = s + table[idx.reshape(-1)][:, :heads].view(n, n, heads).permute(2, 0, 1)
    if mask is not None:
        s = s + mask.to(s.dtype)[None, :, None]
    lse = torch.logsumexp(s, dim=-1)                                     # [B, nw, heads, n]
    o = torch.softmax(s, dim=-1) @ part(v)                               # [B, nw, heads, n, 32]
    o = o.permute(0, 1, 3, 2, 4).reshape(b, nw * n, heads * HEAD_DIM)[:, inv]
    lse = lse.permute(0, 2, 1, 3).reshape(b, heads, nw * n)[:, :, inv]
    return o, lse


def wa_ref(q, k, v, table, do, b, h, w, ws, shift, heads, dtype=torch.float64):
    """the operator at ``dtype`` through autograd -> (O, lse, dQ, dK, dV, dTable [(2 ws - 1)^2, heads])"""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v, table[:, :heads])]
    o, lse = wa_formula(*leaves, b, h, w, ws, shift, heads)
    o.backward(do.to(dtype))
    return (o.detach(), lse.detach()) + tuple(t.grad for t in leaves)


def wa_inputs(b, h, w, ws, heads, dominant, seed):
    """-> q, k, v, dO, the bases of the accumulate run (dQ, dK, dV, dTable), the table"""
    g = torch.Generator().manual_seed(seed)
    c = HEAD_DIM * heads
    q, k, v, do, bq, bk, bv = (torch.randn(b, h * w, c, generator=g) for _ in range(7))
    table = 0.5 * torch.randn(table_rows(ws), heads, generator=g)
    bt = torch.randn(table_rows(ws), heads, generator=g)
    if dominant:
        q = q * 6
    return q, k, v, do, (bq, bk, bv, bt), table


def cell_ln_formula(x, weight, bias, c, cmax, eps=1e-5):
    """x [B, H, W, C], weight / bias [4 Cmax] in transformers' order -> the normalised map [B, H, W, C]: the
    statistics over each 2 x 2 cell's 4 C values, the parameters of phase g = 2 col + row at g * Cmax + c"""
    b, h, w, _ = x.shape
    cells = x.view(b, h // 2, 2, w // 2, 2, c)                          # [b, cy, row, cx, col, c]
    mu = cells.mean(dim=(2, 4, 5), keepdim=True)
    var = ((cells - mu) ** 2).mean(dim=(2, 4, 5), keepdim=True)
    wt = weight.view(2, 2, cmax)[:, :, :c].permute(1, 0, 2)             # [col, row, c] -> [row, col, c]
    bs = bias.view(2, 2, cmax)[:, :, :c].permute(1, 0, 2)
    y = (cells - mu) / torch.sqrt(var + eps) * wt[None, None, :, None] + bs[None, None, :, None]
    return y.reshape(b, h, w, c)


def merge_cat(x):
    """transformers' SwinPatchMerging concatenation of x [B, H, W, C] -> [B, H/2, W/2, 4 C]"""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)


# ---- the backbone --------------------------------------------------------------------------------------
EPS = 1e-5
TINY = dict(depths=[2, 2, 2, 1], num_heads=[2, 2, 3, 2], window_size=7, mlp_ratio=4)
DOUBLING = dict(depths=[2, 2, 2, 1], num_heads=[1, 2, 4, 8], window_size=7, mlp_ratio=4)   # transformers' widths
SUBNETS = {"max": dict(depth=[2, 2, 2, 1], num_heads=[2, 2, 3, 2], mlp_ratio=[4, 4, 4, 4]),
           "sub": dict(depth=[1, 2, 1, 1], num_heads=[1, 2, 2, 1], mlp_ratio=[4, 2, 3, 4])}
DOUBLING_SUBNETS = {"max": dict(depth=[2, 2, 2, 1], num_heads=[1, 2, 4, 8], mlp_ratio=[4, 4, 4, 4]),
                    "sub": dict(depth=[1, 2, 1, 1], num_heads=[1, 2, 4, 8], mlp_ratio=[4, 4, 4, 4])}


def tiny_backbone_cfg(base=TINY, **kw):
    cfg = dict(type="DynamicSwinTransformer", in_channels=3, **base)
    cfg.update(kw)
    return cfg


def randomize_swin(backbone, seed=0):
    """every parameter away from its init (unit norms, zero biases and tiny tables hide mistakes)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in backbone.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and "norm" in name and name.endswith("weight"):
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p[0].numel() ** 0.5))


def swin_ref(sd, x, arch, window_size=7, eps=EPS):
    """The backbone for the subnet ``arch`` from a transformers-layout state dict ``sd`` (any float dtype), on
    an NCHW image x -> the four NCHW features.  Leading slices of every parameter; the merge slices group-wise
    (columns g * Cmax + c, c < C, of its norm and reduction)."""
    import torch.nn.functional as F
    ws = window_size
    heads, depth, ratio = arch["num_heads"], arch["depth"], arch["mlp_ratio"]
    width = [HEAD_DIM * h for h in heads]

    def ln(t, key, c):
        return F.layer_norm(t, (c,), sd[key + ".weight"][:c], sd[key + ".bias"][:c], eps)

    def lin(t, key, co):
        ci = t.shape[-1]
        b = sd.get(key + ".bias")
        return F.linear(t, sd[key + ".weight"][:co, :ci], None if b is None else b[:co])

    p = "swin.embeddings."
    t = F.conv2d(x, sd[p + "patch_embeddings.projection.weight"][:width[0]],
                 sd[p + "patch_embeddings.projection.bias"][:width[0]], stride=4).permute(0, 2, 3, 1)
    t = ln(t, p + "norm", width[0])
    outs = []
    for i in range(4):
        c, b = width[i], t.shape[0]
        hidden = int(ratio[i] * c)
        for j in range(depth[i]):
            k = "swin.encoder.layers.%d.blocks.%d." % (i, j)
            h, w = t.shape[1], t.shape[2]
            hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
            y = F.pad(ln(t, k + "layernorm_before", c), (0, 0, 0, wp - w, 0, hp - h)).reshape(b, hp * wp, c)
            o, _ = wa_formula(lin(y, k + "attention.q_proj", c), lin(y, k + "attention.k_proj", c),
                              lin(y, k + "attention.v_proj", c),
                              sd[k + "attention.relative_position_bias.relative_position_bias_table"],
                              b, hp, wp, ws, 0 if j % 2 == 0 else ws // 2, heads[i])
            o = lin(o, k + "attention.o_proj", c).view(b, hp, wp, c)[:, :h, :w]
            t = t + o
            z = lin(F.gelu(lin(ln(t, k + "layernorm_after", c), k + "mlp.fc1", hidden)), k + "mlp.fc2", c)
            t = t + z
        outs.append(ln(t, "hidden_states_norms.stage%d" % (i + 1), c).permute(0, 3, 1, 2))
        if i < 3:
            k = "swin.encoder.layers.%d.downsample." % i
            cmax = sd[k + "norm.weight"].shape[0] // 4
            cols = torch.cat([torch.arange(g * cmax, g * cmax + c) for g in range(4)])
            m = F.layer_norm(merge_cat(t), (4 * c,), sd[k + "norm.weight"][cols], sd[k + "norm.bias"][cols], eps)
            t = F.linear(m, sd[k + "reduction.weight"][:width[i + 1]][:, cols])
    return outs


def hf_config(base=DOUBLING, arch=None):
    """the SwinConfig of exactly ``arch``'s sizes (head counts must double from stage to stage)"""
    import transformers
    arch = arch or dict(depth=base["depths"], num_heads=base["num_heads"])
    cfg = transformers.SwinConfig(embed_dim=HEAD_DIM * arch["num_heads"][0], depths=list(arch["depth"]),
                                  num_heads=list(arch["num_heads"]), window_size=base["window_size"],
                                  mlp_ratio=base["mlp_ratio"], layer_norm_eps=EPS,
                                  out_features=["stage1", "stage2", "stage3", "stage4"])
    cfg._attn_implementation = "sdpa"
    return cfg
