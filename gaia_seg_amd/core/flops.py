"""Closed-form conv FLOPs / parameters of the active subnet (the analysis the
reference's tools/count_flops.py:118-179 obtains from gaiavision's get_model_complexity_info).

forward FLOPs of a conv = 2 * N * Ho * Wo * Cout_act * Cin_act * kh * kw,
Ho = floor((H + 2p - d(k-1) - 1)/s) + 1.  Only convolutions are counted (BN / ReLU / pooling are
O(activations) and excluded).  For ConvNeXt a depthwise conv counts
2 * K * K * C * Ho * Wo and a DynamicLinear counts as the 1x1 conv it is; LayerNorm, GELU, the layer
scale and ConvNeXt V2's GRN count 0: the reference's counter lives in gaiavision, which is absent, so there is no count of
theirs to reproduce, and they are O(activations) like BN / ReLU above.

For the ElasticTransformer the patch embedding is a conv, every linear counts as the 1x1 conv it is on the N
tokens of an image (cls row included), and self-attention counts 4 * N^2 * 64 * heads per layer and image:
the two matrix products Q K^T and P V at 2 * N^2 * 64 FLOPs per head each.  The softmax (O(N^2) exponentials,
no multiply-add pairs), LayerNorm, GELU and the residual adds count 0.  A DynamicMultiLevelNeck counts its
1x1 and 3x3 convs at the resolutions they run at (key 'neck' of model_flops); the resizes count 0.

The ElasticConvformer follows both conventions: its bottlenecks, projections and patch embedding are convs,
its transformer blocks count as the ElasticTransformer's; the coupling units' LayerNorm, GELU, pooling,
upsample and adds count 0, and the conv-to-token projection counts on the pooled map it runs on.

The DynamicMixVisionTransformer (SegFormer) counts its patch embeddings, reduction convs, linears and the
depthwise 3x3 of the Mix-FFN as the convs they are, and its attention -- Nq tokens of the stage against the Nk
tokens of the reduced map -- 2 x 2 * Nq * Nk * 64 * heads per block and image; the DynamicSegformerHead counts
its 1x1 convs at the sizes they run at.

The DynamicMSCAN (SegNeXt) counts its patch embeddings, 1x1 convs and the depthwise 3x3 of the feed-forward
as the convs they are, and the seven depthwise filters of the spatial gating unit as the depthwise convs they
are (2 * KH * KW * C * H * W each, "same" padding); BatchNorm, LayerNorm, GELU, the gate and the layer scales
count 0."""
from ..hip.ops import conv_out_size
from .bricks import DynamicConv2d


def _conv(m, cin, h, w):
    co = m.width_state
    kh, kw = m.kernel_size
    if m.depthwise:   # one filter per channel: the output width is the input's, one input channel each
        co, cin = cin, 1
    ho = conv_out_size(h, kh, m.stride, m.padding, m.dilation)
    wo = conv_out_size(w, kw, m.stride, m.padding, m.dilation)
    flops = 2.0 * ho * wo * co * cin * kh * kw
    params = co * cin * kh * kw + (co if m.bias is not None else 0)
    return flops, params, co, ho, wo


def convnext_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for a DynamicConvNeXt or a DynamicConvNeXtV2: (flops per image, params, 0.0, feature
    shapes).  Params are those of the extracted subnet: active slices, active blocks, LayerNorm affines and
    layer scales (V1) or the GRN weight and bias of the 4C-wide hidden layer (V2; GRN counts 0 FLOPs)."""
    total, params, c = 0.0, 0.0, in_channels
    f, p, c, h, w = _conv(backbone.stem, c, h, w)
    total += f
    params += p + 2 * c                                   # + the stem LayerNorm
    feats = []
    for i in range(4):
        for blk in backbone.stage(i).active_blocks():
            fd, pd, _, _, _ = _conv(blk.dwconv, c, h, w)
            f1, p1, c1, _, _ = _conv(blk.pwconv1, c, h, w)
            f2, p2, _, _, _ = _conv(blk.pwconv2, c1, h, w)
            total += fd + f1 + f2
            params += pd + p1 + p2 + 2 * c
            params += 2 * c1 if hasattr(blk, "grn") else (c if blk.gamma is not None else 0)
        feats.append((c, h, w))
        if i in backbone.out_indices:
            params += 2 * c                               # norm{i}
        if i < 3:
            params += 2 * c                               # the downsample layer's LayerNorm
            f, p, c, h, w = _conv(getattr(backbone, "ds%d_conv" % (i + 1)), c, h, w)
            total += f
            params += p
    return total, params, 0.0, feats


def attention_flops(n_tokens, heads, head_dim=64):
    """Q K^T and P V of one image: 2 products x 2 * N^2 * head_dim FLOPs per head"""
    return 4.0 * n_tokens * n_tokens * head_dim * heads


def vit_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for an ElasticTransformer: (flops per image, params, 0.0, feature shapes).  Params are
    those of the active subnet's used parameters: patch embedding, tokens, active layers' norms and
    linears (not the relative-position tables or the final norm, which nothing reads)."""
    f, p, d, hp, wp = _conv(backbone.elastic_patch_embed.projection, in_channels, h, w)
    n = hp * wp + 1
    total, params = f, p + d + n * d                      # + cls_token and pos_embed
    feats = []
    for i, name in enumerate(backbone.layers):
        enc = getattr(backbone, name)
        layers = enc.active_layers()
        for layer in layers:
            heads = layer.attn.num_heads
            hw, hidden = 64 * heads, layer.mlp.layer1.width_state
            for cin, cout, count in ((d, hw, 3), (hw, d, 1), (d, hidden, 1), (hidden, d, 1)):
                total += count * 2.0 * n * cin * cout
                params += count * (cin * cout + cout)
            total += attention_flops(n, heads)
            params += 4 * d                               # ln1, ln2
        if i in backbone.out_stages:
            extra = backbone.out_indices[i]
            n_out = 1 if extra is None else 1 + sum(1 for j in extra if j < len(layers))
            feats.extend([(d, hp, wp)] * n_out)
    return total, params, 0.0, feats


def attention_kv_flops(nq, nk, heads, head_dim=64):
    """Q K^T and P V of one image with nq queries and nk keys: 2 products x 2 * nq * nk * head_dim per head"""
    return 4.0 * nq * nk * head_dim * heads


def mit_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for a DynamicMixVisionTransformer: (flops per image, params, 0.0, feature shapes).
    Params are those of the active subnet: active slices, active blocks, LayerNorm affines."""
    total, params, c, feats = 0.0, 0.0, in_channels, []
    for i, stage in enumerate(backbone.stages):
        f, p, c, h, w = _conv(stage.patch_embeddings.proj, c, h, w)
        total += f
        params += p + 2 * c + 2 * c                       # + the embedding's and the stage's LayerNorm
        for blk in stage.active_blocks():
            att, hk, wk = blk.attention, h, w
            params += 4 * c                               # layernorm_before, layernorm_after
            if att.sr_ratio > 1:
                f, p, _, hk, wk = _conv(att.sequence_reduction.sequence_reduction, c, h, w)
                total += f
                params += p + 2 * c
            for lin, (lh, lw) in ((att.q_proj, (h, w)), (att.k_proj, (hk, wk)), (att.v_proj, (hk, wk)),
                                  (att.o_proj, (h, w))):
                f, p, _, _, _ = _conv(lin, c, lh, lw)
                total += f
                params += p
            total += attention_kv_flops(h * w, hk * wk, att.num_heads)
            f1, p1, hidden, _, _ = _conv(blk.mlp.fc1, c, h, w)
            fd, pd, _, _, _ = _conv(blk.mlp.dwconv.dwconv, hidden, h, w)
            f2, p2, _, _, _ = _conv(blk.mlp.fc2, hidden, h, w)
            total += f1 + fd + f2
            params += p1 + pd + p2
        if i in backbone.out_indices:
            feats.append((c, h, w))
    return total, params, 0.0, feats


def mscan_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for a DynamicMSCAN: (flops per image, params, 0.0, feature shapes).  Params are those of
    the active subnet: active slices, active blocks, BatchNorm and LayerNorm affines, layer scales."""
    total, params, c, feats = 0.0, 0.0, in_channels, []
    for i in range(4):
        embed, _, _ = backbone.stage(i)
        for conv in ((embed.proj[0], embed.proj[3]) if i == 0 else (embed.proj,)):
            f, p, c, h, w = _conv(conv, c, h, w)
            total += f
            params += p + 2 * c                           # + the BatchNorm behind it
        params += 2 * c                                   # norm{i}
        for blk in backbone.active_blocks(i):
            sgu = blk.attn.spatial_gating_unit
            params += 2 * 2 * c + 2 * c                   # norm1, norm2, the two layer scales
            for conv in (blk.attn.proj_1, sgu.conv3, blk.attn.proj_2):
                f, p, _, _, _ = _conv(conv, c, h, w)
                total += f
                params += p
            for dw in sgu.depthwise():
                kh, kw = dw.kernel_size
                total += 2.0 * kh * kw * c * h * w
                params += kh * kw * c + c
            f1, p1, hidden, _, _ = _conv(blk.mlp.fc1, c, h, w)
            fd, pd, _, _, _ = _conv(blk.mlp.dwconv, hidden, h, w)
            f2, p2, _, _, _ = _conv(blk.mlp.fc2, hidden, h, w)
            total += f1 + fd + f2
            params += p1 + pd + p2
        if i in backbone.out_indices:
            feats.append((c, h, w))
    return total, params, 0.0, feats


def swin_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for a DynamicSwinTransformer: (flops per image, params, 0.0, feature shapes).  It counts
    what runs: q / k / v and the attention on the map padded to the window (every token attends to ws^2 keys: 2
    products x 2 * Hp Wp * ws^2 * 32 heads), o_proj and the MLP on the cropped map, the merge as its 2x2 stride-2
    conv.  (Published Swin counts put o_proj on the padded map too; here it runs after the crop, so its term is
    smaller wherever a stage pads.)  Params are those of the active subnet (swin.layernorm, which nothing reads,
    is not counted)."""
    ws = backbone.window_size
    emb = backbone.swin.embeddings
    total, params, c, h, w = _conv(emb.patch_embeddings.projection, in_channels, h, w)
    params += 2 * c                                       # embeddings.norm
    feats = []
    for i, stage in enumerate(backbone.stages):
        hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
        for blk in stage.active_blocks():
            att = blk.attention
            params += 4 * c + (2 * ws - 1) ** 2 * att.num_heads      # the two LayerNorms, the table's active part
            for lin, (lh, lw) in ((att.q_proj, (hp, wp)), (att.k_proj, (hp, wp)), (att.v_proj, (hp, wp)),
                                  (att.o_proj, (h, w))):
                f, p, _, _, _ = _conv(lin, c, lh, lw)
                total += f
                params += p
            total += 4.0 * hp * wp * ws * ws * 32 * att.num_heads
            f1, p1, hidden, _, _ = _conv(blk.mlp.fc1, c, h, w)
            f2, p2, _, _, _ = _conv(blk.mlp.fc2, hidden, h, w)
            total += f1 + f2
            params += p1 + p2
        if i in backbone.out_indices:
            feats.append((c, h, w))
            params += 2 * c                               # hidden_states_norms.stage{i+1}
        if stage.downsample is not None:
            params += 2 * 4 * c                           # the merge's LayerNorm over 4 C
            f, p, c, h, w = _conv(stage.downsample.reduction, c, h, w)
            total += f
            params += p
    return total, params, 0.0, feats


def _trans_block(blk, n, d):
    """(flops per image, params) of an Elastic_trans_Block on n tokens of width d"""
    heads = blk.attn.num_heads
    hw, hidden = 64 * heads, blk.mlp.layer1.width_state
    total, params = attention_flops(n, heads), 4 * d       # ln1, ln2
    for cin, cout, count in ((d, hw, 3), (hw, d, 1), (d, hidden, 1), (hidden, d, 1)):
        total += count * 2.0 * n * cin * cout
        params += count * (cin * cout + cout)
    return total, params


def _conv_block(blk, c, h, w):
    """(flops, params, flops of the 3x3, output width, height, width) of an Elastic_conv_Block"""
    f1, p1, c1, _, _ = _conv(blk.conv1, c, h, w)
    f2, p2, c2, h2, w2 = _conv(blk.conv2, c1, h, w)
    f3, p3, c3, _, _ = _conv(blk.conv3, c2, h2, w2)
    total, params = f1 + f2 + f3, p1 + p2 + p3 + 2 * (c1 + c2 + c3)
    if blk.res_conv:
        fr, pr, cr, _, _ = _conv(blk.residual_conv, c, h, w)
        total += fr
        params += pr + 2 * cr
    return total, params, f2, c3, h2, w2


def convformer_backbone_flops(backbone, h, w, in_channels=3):
    """backbone_flops for an ElasticConvformer: (flops per image, params, flops of the 3x3 convs, feature
    shapes).  Convs and linears count, attention counts 4 * N^2 * 64 * heads; norms, GELU, pooling, the
    upsample and the adds count 0.  The conv-to-token projection is counted on the POOLED map, as it is
    executed.  Params are those of the active subnet's used parameters."""
    f, p, c, h, w = _conv(backbone.conv1, in_channels, h, w)
    total, params, k3 = f, p + 2 * c, 0.0
    mp = backbone.maxpool
    h = (h + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    w = (w + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    feats, n, d = [], None, None
    for name in backbone.layers:
        for blk in getattr(backbone, name).active_blocks():
            if blk.stage:
                fp, pp, d, hp, wp = _conv(blk.trans_patch_conv, c, h, w)
                n = hp * wp + 1
                ft, pt = _trans_block(blk.trans_1, n, d)
                fc, pc, f3, c, h, w = _conv_block(blk.conv_1, c, h, w)
                total += fp + ft + fc
                params += pp + pt + pc + d                  # + cls_token
                k3 += f3
                continue
            fc, pc, f3, c, h, w = _conv_block(blk.cnn_block, c, h, w)
            s, med = blk.dw_stride, blk.cnn_block.conv2.width_state
            fs, ps, _, _, _ = _conv(blk.squeeze_block.conv_project, med, h // s, w // s)
            ft, pt = _trans_block(blk.trans_block, n, d)
            fe, pe, ce, _, _ = _conv(blk.expand_block.conv_project, d, h // s, w // s)
            ff, pf, f3f, c, h, w = _conv_block(blk.fusion_block, c, h, w)
            total += fc + fs + ft + fe + ff
            params += pc + ps + 2 * d + pt + pe + 2 * ce + pf
            k3 += f3 + f3f
        feats.append((c, h, w))
    return total, params, k3, feats


def neck_flops(neck, feats):
    """DynamicMultiLevelNeck: (flops per image, feature shapes after the neck)"""
    from ..models.necks.dynamic_multilevel_neck import scaled_size
    total, laterals = 0.0, []
    for (c, h, w), lat in zip(feats, neck.lateral_convs):
        f, _, co, _, _ = _conv(lat.conv, c, h, w)
        total += f
        laterals.append((co, h, w))
    if len(laterals) == 1:
        laterals = laterals * neck.num_outs
    out = []
    for (c, h, w), scale, conv in zip(laterals, neck.scales, neck.convs):
        h, w = scaled_size(h, scale), scaled_size(w, scale)
        f, _, co, _, _ = _conv(conv.conv, c, h, w)
        total += f
        out.append((co, h, w))
    return total, out


def backbone_flops(backbone, h, w, in_channels=3):
    """(flops per image, params, flops of the 3x3 bottleneck convs, feature shapes)."""
    if type(backbone).__name__ in ("DynamicConvNeXt", "DynamicConvNeXtV2"):
        return convnext_backbone_flops(backbone, h, w, in_channels)
    if type(backbone).__name__ == "ElasticTransformer":
        return vit_backbone_flops(backbone, h, w, in_channels)
    if type(backbone).__name__ == "ElasticConvformer":
        return convformer_backbone_flops(backbone, h, w, in_channels)
    if type(backbone).__name__ == "DynamicMixVisionTransformer":
        return mit_backbone_flops(backbone, h, w, in_channels)
    if type(backbone).__name__ == "DynamicSwinTransformer":
        return swin_backbone_flops(backbone, h, w, in_channels)
    if type(backbone).__name__ == "DynamicMSCAN":
        return mscan_backbone_flops(backbone, h, w, in_channels)
    total = params = k3 = 0.0
    c = in_channels
    if backbone.deep_stem:
        for i in (0, 3, 6):
            f, p, c, h, w = _conv(backbone.stem[i], c, h, w)
            total += f
            params += p + 2 * c
    else:
        f, p, c, h, w = _conv(backbone.conv1, c, h, w)
        total += f
        params += p + 2 * c
    mp = backbone.maxpool
    h = (h + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    w = (w + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    feats = []
    for name in backbone.res_layers:
        layer = getattr(backbone, name)
        for blk in layer.active_blocks():
            cin = c
            f1, p1, c1, h1, w1 = _conv(blk.conv1, cin, h, w)
            f2, p2, c2, h2, w2 = _conv(blk.conv2, c1, h1, w1)
            f3, p3, c3, h3, w3 = _conv(blk.conv3, c2, h2, w2)
            total += f1 + f2 + f3
            k3 += f2
            params += p1 + p2 + p3 + 2 * (c1 + c2 + c3)
            if blk.downsample is not None:
                for m in blk.downsample:
                    if isinstance(m, DynamicConv2d):
                        fd, pd, cd, _, _ = _conv(m, cin, h, w)
                        total += fd
                        params += pd + 2 * cd
            c, h, w = c3, h3, w3
        feats.append((c, h, w))
    return total, params, k3, feats


def fcn_head_flops(head, c, h, w):
    total = 0.0
    x_c = c
    mods = [] if head.num_convs == 0 else list(head.convs)
    for m in mods:
        f, _, c, h, w = _conv(m.conv, c, h, w)
        total += f
    if head.concat_input:
        f, _, c, h, w = _conv(head.conv_cat.conv, x_c + c, h, w)
        total += f
    f, _, _, _, _ = _conv(head.conv_seg, c, h, w)
    return total + f


def psp_head_flops(head, c, h, w):
    total = 0.0
    for s, ppm in zip(head.pool_scales, head.psp_modules):
        f, _, _, _, _ = _conv(ppm[1].conv, c, s, s)
        total += f
    f, _, cb, _, _ = _conv(head.bottleneck.conv, c + len(head.pool_scales) * head.channels, h, w)
    total += f
    f, _, _, _, _ = _conv(head.conv_seg, cb, h, w)
    return total + f


def _conv_module(m, c, h, w):
    """(flops, output width) of a DynamicConvModule or DynamicDepthwiseSeparableConvModule."""
    if hasattr(m, "depthwise_conv"):
        fd, _, c, h, w = _conv(m.depthwise_conv.conv, c, h, w)
        fp, _, c, _, _ = _conv(m.pointwise_conv.conv, c, h, w)
        return fd + fp, c
    f, _, c, _, _ = _conv(m.conv, c, h, w)
    return f, c


def aspp_head_flops(head, feats):
    """DynamicASPPHead / DynamicDepthwiseSeparableASPPHead: the image-pool 1x1 conv on one pixel, one
    branch per dilation and the 3x3 bottleneck at the input's size; for DeepLabV3+ also the 1x1
    c1_bottleneck and the two separable convs at the first level's size, where the classifier then
    runs."""
    c, h, w = feats[head.in_index % len(feats)]
    total = _conv_module(head.image_pool[1], c, 1, 1)[0]
    for m in head.aspp_modules:
        total += _conv_module(m, c, h, w)[0]
    f, cb = _conv_module(head.bottleneck, (len(head.dilations) + 1) * head.channels, h, w)
    total += f
    if hasattr(head, "sep_bottleneck"):
        if head.c1_bottleneck is not None:
            c1, h, w = feats[0]
            f, c1 = _conv_module(head.c1_bottleneck, c1, h, w)
            total += f
            cb += c1
        for m in head.sep_bottleneck:
            f, cb = _conv_module(m, cb, h, w)
            total += f
    return total + _conv(head.conv_seg, cb, h, w)[0]


def uper_head_flops(head, feats):
    """DynamicUPerHead (gaiaseg/models/decode_heads/dynamic_uper_head.py:81-131): PPM + bottleneck on
    the last level, one 1x1 lateral and one 3x3 fpn conv per other level at that level's size, the
    3x3 fpn_bottleneck over the concatenated levels and the classifier at the first level's size."""
    levels = [feats[i] for i in head.in_index]
    c5, h5, w5 = levels[-1]
    total = 0.0
    scales = head.psp_modules.pool_scales
    for s, ppm in zip(scales, head.psp_modules):
        total += _conv(ppm[1].conv, c5, s, s)[0]
    total += _conv(head.bottleneck.conv, c5 + len(scales) * head.channels, h5, w5)[0]
    for (c, h, w), lat, fpn in zip(levels[:-1], head.lateral_convs, head.fpn_convs):
        total += _conv(lat.conv, c, h, w)[0]
        total += _conv(fpn.conv, head.channels, h, w)[0]
    _, h0, w0 = levels[0]
    f, _, cb, _, _ = _conv(head.fpn_bottleneck.conv, len(levels) * head.channels, h0, w0)
    return total + f + _conv(head.conv_seg, cb, h0, w0)[0]


def segformer_head_flops(head, feats):
    """DynamicSegformerHead: one 1x1 conv per level at that level's size, the 1x1 fusion conv over the
    concatenated levels and the classifier at the first level's size; the resizes count 0."""
    levels = [feats[i] for i in head.in_index]
    total = sum(_conv(m.conv, c, h, w)[0] for (c, h, w), m in zip(levels, head.convs))
    _, h0, w0 = levels[0]
    f, _, cb, _, _ = _conv(head.fusion_conv.conv, len(levels) * head.channels, h0, w0)
    return total + f + _conv(head.conv_seg, cb, h0, w0)[0]


def ocr_head_flops(head, feats, num_prev_classes=None):
    """DynamicOCRHead: the 3x3 bottleneck, the two query projections, the output projection, the 1x1
    bottleneck over the concat buffer and the classifier at the input's P = h * w pixels; the two key
    projections and the value projection on the K x 1 region map.  Convs count as everywhere (2 FLOPs per
    multiply-add).  The two region products count K * P * C multiply-adds for the gather (2 * K * P * C
    FLOPs) and 2 * K * P * ch for the attention (scores and weighted values: 4 * K * P * ch FLOPs);
    softmax exponentials are not counted.  K is the class count of the previous head's logits."""
    c, h, w = feats[head.in_index % len(feats)]
    k = head.num_classes if num_prev_classes is None else num_prev_classes
    ocb = head.object_context_block
    total, ch = _conv_module(head.bottleneck, c, h, w)
    total += 2.0 * k * h * w * ch
    cq = ch
    for m in ocb.query_project:
        f, cq = _conv_module(m, cq, h, w)
        total += f
    ck = ch
    for m in ocb.key_project:
        f, ck = _conv_module(m, ck, k, 1)
        total += f
    total += _conv_module(ocb.value_project, ch, k, 1)[0]
    total += 4.0 * k * h * w * cq
    f, co = _conv_module(ocb.out_project, cq, h, w)
    total += f
    f, cb = _conv_module(ocb.bottleneck, co + ch, h, w)
    return total + f + _conv(head.conv_seg, cb, h, w)[0]


def _head_flops(head, feats, prev=None):
    name = type(head).__name__
    if isinstance(head.in_index, int):
        c, fh, fw = feats[head.in_index % len(feats)]
    if name == "DynamicFCNHead":
        return fcn_head_flops(head, c, fh, fw)
    if name == "DynamicPSPHead":
        return psp_head_flops(head, c, fh, fw)
    if name == "DynamicUPerHead":
        return uper_head_flops(head, feats)
    if name == "DynamicSegformerHead":
        return segformer_head_flops(head, feats)
    if name in ("DynamicASPPHead", "DynamicDepthwiseSeparableASPPHead"):
        return aspp_head_flops(head, feats)
    if name == "DynamicOCRHead":
        return ocr_head_flops(head, feats, prev.num_classes if prev is not None else None)
    return float("nan")


def model_flops(model, h, w):
    """dict(backbone, backbone_3x3, [neck,] decode, aux, total) in FLOPs per image for the current arch.
    A cascade of decode heads (DynamicCascadeEncoderDecoder) adds one ``decode_<i>`` entry per stage;
    ``decode`` is their sum."""
    import torch.nn as nn
    b, params, k3, feats = backbone_flops(model.backbone, h, w)
    out = dict(backbone=b, backbone_3x3=k3, backbone_params=params)
    if getattr(model, "neck", None) is not None:
        out["neck"], feats = neck_flops(model.neck, feats)
    for key, head in (("decode", model.decode_head), ("aux", getattr(model, "auxiliary_head", None))):
        if head is None:
            continue
        if key == "decode" and isinstance(head, nn.ModuleList):
            prev = None
            for i, stage in enumerate(head):
                out["decode_%d" % i] = _head_flops(stage, feats, prev)
                prev = stage
            out[key] = sum(out["decode_%d" % i] for i in range(len(head)))
        else:
            out[key] = _head_flops(head, feats)
    out["total"] = sum(v for k, v in out.items() if k in ("backbone", "neck", "decode", "aux") and v == v)
    return out
