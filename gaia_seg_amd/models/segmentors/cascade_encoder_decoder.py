"""CascadeEncoderDecoder / DynamicCascadeEncoderDecoder — a segmentor whose decode heads form a cascade:
head i takes the backbone features AND the logits of head i - 1 (mmseg's CascadeEncoderDecoder,
mmseg/models/segmentors/cascade_encoder_decoder.py; OCRNet is FCNHead -> OCRHead).

``decode_head`` is a list of ``num_stages`` configs and becomes an ``nn.ModuleList``: state-dict keys are
``decode_head.0.*``, ``decode_head.1.*`` as in mmseg.  ``align_corners`` and ``num_classes`` come from the
last head.  Only the four decode-head hooks of EncoderDecoder are overridden; the inference epilogue, TTA,
BatchNorm re-calibration, subnet extraction and the evaluation hooks all go through
``_decode_head_forward_test`` and work unchanged.

Training: stage i's losses carry the prefix ``decode_i``; stage i > 0 reads the logits of stage i - 1 WITH
their gradient (the soft regions feed back into the previous head).  One departure from mmseg: stage i - 1
runs ONCE and its logits serve both its own loss and the next stage.  mmseg runs it a second time through
``forward_test``, which is the same when ``dropout_ratio=0``; otherwise its two runs draw different
dropout masks.

In-place distillation (teacher logits in the training kwargs) and a fixed teacher (DynamicDistiller) are
out of scope with a cascade and refused where met."""
import torch.nn as nn

from .. import builder
from ..builder import SEGMENTORS
from .dynamic_encoder_decoder import DynamicEncoderDecoder
from .encoder_decoder import EncoderDecoder, add_prefix


class _CascadeMixin:
    """the four decode-head hooks of EncoderDecoder for a list of heads"""

    def _init_decode_head(self, decode_head):
        if not isinstance(decode_head, (list, tuple)) or len(decode_head) != self.num_stages:
            raise ValueError("%s: decode_head must be a list of num_stages=%d head configs"
                             % (type(self).__name__, self.num_stages))
        self.decode_head = nn.ModuleList([builder.build_head(h) for h in decode_head])
        self.align_corners = self.decode_head[-1].align_corners
        self.num_classes = self.decode_head[-1].num_classes

    def init_weights(self, pretrained=None):
        self.backbone.init_weights(pretrained=pretrained)
        for head in self.decode_head:
            head.init_weights()
        if self.with_auxiliary_head:
            aux = self.auxiliary_head
            for head in (aux if isinstance(aux, nn.ModuleList) else [aux]):
                head.init_weights()

    def _decode_head_forward_train(self, x, img_metas, gt_semantic_seg, **kwargs):
        if any(kwargs.get(k) is not None for k in ("teacher_logits", "aux_teacher_logits")) \
                or kwargs.get("return_logits"):
            raise NotImplementedError("%s: in-place distillation with a cascade of decode heads is not "
                                      "supported" % type(self).__name__)
        losses = dict()
        prev = None
        for i, head in enumerate(self.decode_head):
            logits = head.forward(x) if i == 0 else head.forward(x, prev)
            losses.update(add_prefix(head.losses(logits, gt_semantic_seg), "decode_%d" % i))
            prev = logits
        return losses

    def _decode_head_forward_test(self, x, img_metas):
        out = self.decode_head[0].forward_test(x, img_metas, self.test_cfg)
        for head in list(self.decode_head)[1:]:
            out = head.forward_test(x, out, img_metas, self.test_cfg)
        return out


@SEGMENTORS.register_module()   # (a fixed model by its mmseg name, as EncoderDecoder is)
class CascadeEncoderDecoder(_CascadeMixin, EncoderDecoder):
    def __init__(self, num_stages, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None,
                 test_cfg=None, pretrained=None):
        self.num_stages = num_stages
        super().__init__(backbone=backbone, decode_head=decode_head, neck=neck,
                         auxiliary_head=auxiliary_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained)


@SEGMENTORS.register_module()
class DynamicCascadeEncoderDecoder(_CascadeMixin, DynamicEncoderDecoder):
    """The search-space root with a cascade of heads: ``arch['backbone']`` goes to the backbone, the
    heads follow the feature widths (DynamicEncoderDecoder); ``active_parameters()`` covers every head."""

    def __init__(self, num_stages, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None,
                 test_cfg=None, pretrained=None):
        self.num_stages = num_stages
        super().__init__(backbone=backbone, decode_head=decode_head, neck=neck,
                         auxiliary_head=auxiliary_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained)
