"""DynamicOCRHead — OCRNet's decode head (Yuan et al., "Object-Contextual Representations for Semantic
Segmentation") with dynamic input widths, after mmseg's OCRHead (mmseg/models/decode_heads/ocr_head.py:
SpatialGatherModule, ObjectAttentionBlock over mmseg/models/utils/self_attention_block.py) and
BaseCascadeDecodeHead (cascade_decode_head.py).

The reference tree has no such head; it completes the mainstream Cityscapes families on the OS8 / v1c
supernet (configs/supernet/ocrnet_ar50to101_v1c_os8.py).  It is the second stage of a
DynamicCascadeEncoderDecoder: its forward takes the previous head's logits, which define the soft
object regions.  ``in_channels`` is the supernet maximum; the bottleneck slices its weight to the
feature map's channel count (DynConv2d semantics), so the head needs no search space of its own.

    feats   = bottleneck(x)                                   3x3, into slice [ch, 2ch) of the concat buffer
    context = ocr_gather(feats, prev_output, scale)           [B, K, channels] as a K x 1 map
    q = query_project(feats); k = key_project(context); v = value_project(context)
    obj     = out_project(ocr_attend(q, k, v))                into slice [0, ch) of the concat buffer
    out     = cls_seg(object_context_block.bottleneck(cat))   cat = [obj, feats], never copied

The two products (csrc/ocr.hip) are HIP operators of their own; everything else is a DynamicConvModule.
State-dict keys are mmseg's, so the head of an mmseg OCRNet checkpoint loads by name.

Out of scope, refused where met: ``scale != 1`` (mmseg max-pools the queries by it), an
``input_transform``, and teacher logits (the head has no in-place distillation branch)."""
import torch
import torch.nn as nn

from ...core.bricks import DynamicConvModule
from ...hip import ops
from ...hip.runtime import Act, tape_function
from ..builder import HEADS
from .decode_head import DynamicBaseDecodeHead


class DynamicObjectAttentionBlock(nn.Module):
    """mmseg's ObjectAttentionBlock at scale 1: query / key projections of two 1x1 conv-BN-ReLU, value and
    output projections of one, and the 1x1 bottleneck over cat([context, query_feats])."""

    def __init__(self, in_channels, channels, conv_cfg, norm_cfg, act_cfg):
        super().__init__()
        self.in_channels, self.channels = in_channels, channels

        def proj(cin, cout):
            return DynamicConvModule(cin, cout, 1, conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)
        self.query_project = nn.Sequential(proj(in_channels, channels), proj(channels, channels))
        self.key_project = nn.Sequential(proj(in_channels, channels), proj(channels, channels))
        self.value_project = proj(in_channels, channels)
        self.out_project = proj(channels, in_channels)
        self.bottleneck = proj(2 * in_channels, in_channels)

    def forward_acts(self, tape, cat, feats, context):
        """cat: the [B, H, W, 2 * in_channels] buffer whose upper half ``feats`` is; context: the region map"""
        q = k = None
        for m in self.query_project:
            q = m.forward_act(tape, feats if q is None else q)
        for m in self.key_project:
            k = m.forward_act(tape, context if k is None else k)
        v = self.value_project.forward_act(tape, context)
        self.out_project.forward_act(tape, ops.ocr_attend(tape, q, k, v), out=cat.slice(0, self.in_channels))
        return self.bottleneck.forward_act(tape, cat)


@HEADS.register_module()
class DynamicOCRHead(DynamicBaseDecodeHead):
    def __init__(self, ocr_channels, in_channels, channels, num_classes, scale=1, dropout_ratio=0.1,
                 conv_cfg=None, norm_cfg=None, act_cfg=dict(type="ReLU"), in_index=-1, input_transform=None,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                 ignore_index=255, sampler=None, align_corners=False):
        super().__init__(in_channels, channels, num_classes=num_classes, dropout_ratio=dropout_ratio,
                         conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg, in_index=in_index,
                         input_transform=input_transform, loss_decode=loss_decode,
                         ignore_index=ignore_index, sampler=sampler, align_corners=align_corners)
        if input_transform is not None:
            raise NotImplementedError("%s takes one feature map (input_transform=None)" % type(self).__name__)
        if scale != 1:
            raise NotImplementedError("%s supports scale=1 only: scale > 1 max-pools the queries and is out "
                                      "of scope" % type(self).__name__)
        self.ocr_channels, self.scale = ocr_channels, scale
        self.object_context_block = DynamicObjectAttentionBlock(
            self.channels, self.ocr_channels, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
            act_cfg=self.act_cfg)
        self.bottleneck = DynamicConvModule(self.in_channels, self.channels, 3, padding=1,
                                            conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                            act_cfg=self.act_cfg)

    def ocr_concat(self, tape, x, prev):
        """cat([object context, feats], dim=1) without materialising the pieces: the concat buffer"""
        ch = self.channels
        cat = Act.empty(x.N, x.H, x.W, 2 * ch, x.t.device)
        feats = self.bottleneck.forward_act(tape, x, out=cat.slice(ch, 2 * ch))
        context = ops.ocr_gather(tape, feats, prev, float(self.scale))
        return cat, feats, context

    def forward_acts(self, tape, x, prev=None):
        cat, feats, context = self.ocr_concat(tape, x, prev)
        return self.cls_seg_act(tape, self.object_context_block.forward_acts(tape, cat, feats, context))

    def forward(self, inputs, prev_output):
        inputs = list(inputs)
        x = inputs[self.in_index % len(inputs)]
        if tuple(prev_output.shape[2:]) != tuple(x.shape[2:]):
            # (mmseg fails in the gather's matmul: both heads must read stages of one stride)
            raise ValueError("%s: the previous head's logits are %d x %d, the selected feature map %d x %d; "
                             "both heads must read stages of one stride (OS8 supernet)"
                             % ((type(self).__name__,) + tuple(prev_output.shape[2:]) + tuple(x.shape[2:])))
        if prev_output.stride(3) == 1 and prev_output.shape[1] % 4:
            # (a packed NCHW map of a width that is no float4 multiple would be taken for an image)
            prev_output = prev_output.contiguous(memory_format=torch.channels_last)
        needs = any(p.requires_grad for p in self.parameters())

        def runner(tape, acts):
            return [self.forward_acts(tape, acts[0], acts[1])]
        return tape_function(runner, [x, prev_output], needs)[0]

    # ---- mmseg's BaseCascadeDecodeHead ----
    def forward_train(self, inputs, prev_output, img_metas, gt_semantic_seg, train_cfg, **kwargs):
        if any(kwargs.get(k) is not None for k in ("teacher_logits", "aux_teacher_logits")):
            raise NotImplementedError(
                "%s has no in-place distillation branch (its reference forward_train takes no teacher "
                "logits)" % type(self).__name__)
        return self.losses(self.forward(inputs, prev_output), gt_semantic_seg)

    def forward_test(self, inputs, prev_output, img_metas, test_cfg):
        return self.forward(inputs, prev_output)
