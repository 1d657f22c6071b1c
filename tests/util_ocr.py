"""CPU restatement of OCRNet in plain torch (float64 after ``.double()``), written from mmseg's
SpatialGatherModule / ObjectAttentionBlock / OCRHead (mmseg/models/decode_heads/ocr_head.py over
mmseg/models/utils/self_attention_block.py), FCNHead and CascadeEncoderDecoder's training flow: what
tests/test_ocr*.py compare the HIP operators, the DynamicOCRHead and the cascade segmentor against.

The modules carry the state-dict keys of the product heads (``load_state_dict(strict=True)`` of a product
head's state works) and the dynamic-width rule of tests/util_aspp.py's bricks."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from util_aspp import RefConv, RefConvModule, count_macs, load_into_ref  # noqa: F401


# ---- the two operators as functions (what the C-ABI tests check) -----------------------------------
def spatial_gather(feats, probs, scale=1.0):
    """SpatialGatherModule.forward: feats [B, C, H, W], probs [B, K, H, W] -> context [B, C, K, 1]"""
    b, k = probs.shape[:2]
    c = feats.size(1)
    probs = F.softmax(scale * probs.reshape(b, k, -1), dim=2)
    feats = feats.reshape(b, c, -1).permute(0, 2, 1)
    return torch.matmul(probs, feats).permute(0, 2, 1).contiguous().unsqueeze(3)


def object_attention(query, key, value):
    """the matmul core of SelfAttentionBlock.forward with matmul_norm: query [B, P, ch], key and value
    [B, K, ch] -> [B, P, ch]"""
    sim = torch.matmul(query, key.transpose(1, 2)) * query.size(2) ** -0.5
    return torch.matmul(F.softmax(sim, dim=-1), value)


def gather_ref(logits, feats, scale, dctx):
    """float64 gather on rows-x-C operands: logits [B, P, K], feats [B, P, C], dctx [B, K, C] ->
    (ctx [B, K, C], stats [B, K, 2] = (max, log sum), dfeats, dlogits)"""
    lg = logits.double().requires_grad_(True)
    ft = feats.double().requires_grad_(True)
    w = F.softmax(scale * lg.transpose(1, 2), dim=2)             # [B, K, P]
    ctx = torch.matmul(w, ft)
    ctx.backward(dctx.double())
    x = scale * logits.double().transpose(1, 2)
    m = x.max(dim=2).values
    stats = torch.stack([m, torch.log(torch.exp(x - m.unsqueeze(2)).sum(dim=2))], dim=2)
    return ctx.detach(), stats, ft.grad, lg.grad


def attend_ref(q, k, v, dout):
    """float64 attend: q [B, P, ch], k, v [B, K, ch], dout [B, P, ch] -> (out, lse [B, P], dq, dk, dv)"""
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    out = object_attention(q, k, v)
    out.backward(dout.double())
    sim = torch.matmul(q.detach(), k.detach().transpose(1, 2)) * q.size(2) ** -0.5
    return out.detach(), torch.logsumexp(sim, dim=2), q.grad, k.grad, v.grad


# ---- the heads --------------------------------------------------------------------------------------
class RefObjectAttentionBlock(nn.Module):
    def __init__(self, in_channels, channels):
        super().__init__()
        self.channels = channels
        self.query_project = nn.Sequential(RefConvModule(in_channels, channels, 1),
                                           RefConvModule(channels, channels, 1))
        self.key_project = nn.Sequential(RefConvModule(in_channels, channels, 1),
                                         RefConvModule(channels, channels, 1))
        self.value_project = RefConvModule(in_channels, channels, 1)
        self.out_project = RefConvModule(channels, in_channels, 1)
        self.bottleneck = RefConvModule(2 * in_channels, in_channels, 1)

    def context(self, query_feats, key_feats):
        b = query_feats.size(0)
        query = self.query_project(query_feats).reshape(b, self.channels, -1).permute(0, 2, 1)
        key = self.key_project(key_feats).reshape(b, self.channels, -1).permute(0, 2, 1)
        value = self.value_project(key_feats).reshape(b, self.channels, -1).permute(0, 2, 1)
        ctx = object_attention(query, key, value).permute(0, 2, 1).contiguous()
        return self.out_project(ctx.reshape(b, self.channels, *query_feats.shape[2:]))

    def forward(self, query_feats, key_feats):
        return self.bottleneck(torch.cat([self.context(query_feats, key_feats), query_feats], dim=1))


class _RefHead(nn.Module):
    def __init__(self, channels, num_classes, in_index, loss_weight, align_corners=False, ignore_index=255):
        super().__init__()
        self.in_index, self.num_classes = in_index, num_classes
        self.loss_weight, self.align_corners, self.ignore_index = loss_weight, align_corners, ignore_index
        self.conv_seg = RefConv(channels, num_classes, 1, bias=True)

    def losses(self, seg_logit, seg_label):
        from oracle import ops as O
        return O.seg_losses(seg_logit, seg_label, self.loss_weight, self.ignore_index, self.align_corners,
                            None, None)


class RefFCNHead(_RefHead):
    """FCNHead with num_convs 3x3 conv modules and no concat_input"""

    def __init__(self, in_channels, channels, num_classes, num_convs=1, in_index=-1, loss_weight=1.0):
        super().__init__(channels, num_classes, in_index, loss_weight)
        self.convs = nn.Sequential(*[RefConvModule(in_channels if i == 0 else channels, channels, 3, 1)
                                     for i in range(num_convs)])

    def forward(self, inputs):
        return self.conv_seg(self.convs(inputs[self.in_index]))


class RefOCRHead(_RefHead):
    def __init__(self, in_channels, channels, ocr_channels, num_classes, scale=1, in_index=-1, loss_weight=1.0):
        super().__init__(channels, num_classes, in_index, loss_weight)
        self.scale = scale
        self.object_context_block = RefObjectAttentionBlock(channels, ocr_channels)
        self.bottleneck = RefConvModule(in_channels, channels, 3, 1)

    def forward(self, inputs, prev_output):
        feats = self.bottleneck(inputs[self.in_index])
        context = spatial_gather(feats, prev_output, self.scale)
        return self.conv_seg(self.object_context_block(feats, context))


class RefCascade(nn.Module):
    """the decode heads of CascadeEncoderDecoder over given backbone features; keys decode_head.<i>.*"""

    def __init__(self, heads):
        super().__init__()
        self.decode_head = nn.ModuleList(heads)

    def forward(self, inputs):
        """every stage's logits"""
        outs = [self.decode_head[0](inputs)]
        for head in list(self.decode_head)[1:]:
            outs.append(head(inputs, outs[-1]))
        return outs

    def forward_train(self, inputs, gt):
        """(losses with CascadeEncoderDecoder's prefixes, every stage's logits); stage i reads the logits of
        stage i - 1 with their gradient"""
        outs = self.forward(inputs)
        losses = {}
        for i, (head, out) in enumerate(zip(self.decode_head, outs)):
            for k, v in head.losses(out, gt).items():
                losses["decode_%d.%s" % (i, k)] = v
        return losses, outs


# ---- the tiny cascade the tests use (the tiny supernet's stage widths are maxima: 384 and 512) --------
TINY_FCN = dict(in_channels=384, channels=16, num_classes=19, num_convs=1, in_index=2)
TINY_OCR = dict(in_channels=512, channels=16, ocr_channels=8, num_classes=19, in_index=3)
NORM = dict(type="SyncBN", requires_grad=True)


def fcn_cfg(dropout=0.0, loss_weight=0.4, **over):
    cfg = dict(type="DynamicFCNHead", conv_cfg=dict(type="DynConv2d"), concat_input=False, dropout_ratio=dropout,
               norm_cfg=dict(NORM), align_corners=False,
               loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=loss_weight), **TINY_FCN)
    cfg.update(over)
    return cfg


def ocr_cfg(dropout=0.0, loss_weight=1.0, **over):
    cfg = dict(type="DynamicOCRHead", conv_cfg=dict(type="DynConv2d"), dropout_ratio=dropout,
               norm_cfg=dict(NORM), align_corners=False,
               loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=loss_weight), **TINY_OCR)
    cfg.update(over)
    return cfg


def cascade_cfg(dropout=0.0, ocr_loss_weight=1.0):
    """the tiny cascade model on the tiny OS8 / v1c backbone of tests/util_models.py"""
    from util_models import tiny_backbone
    return dict(type="DynamicCascadeEncoderDecoder", num_stages=2, backbone=tiny_backbone(os8=True),
                decode_head=[fcn_cfg(dropout), ocr_cfg(dropout, ocr_loss_weight)], train_cfg=dict(),
                test_cfg=dict(mode="whole"))


def ref_cascade(fcn_loss_weight=0.4, ocr_loss_weight=1.0):
    return RefCascade([RefFCNHead(loss_weight=fcn_loss_weight, **TINY_FCN),
                       RefOCRHead(loss_weight=ocr_loss_weight, **TINY_OCR)])


def count_ocr_macs(cascade, inputs):
    """multiply-adds per image of one forward of a RefCascade: every conv by forward hooks (util_aspp's
    count), plus the two region products, K * P * C for the gather and 2 * K * P * ch for the attention"""
    macs = count_macs(cascade, inputs)
    for head in cascade.decode_head:
        if isinstance(head, RefOCRHead):
            x = inputs[head.in_index]
            p = x.size(2) * x.size(3)
            k = head.num_classes
            c = head.bottleneck.conv.weight.size(0)
            ch = head.object_context_block.channels
            macs += k * p * c + 2 * k * p * ch
    return macs
