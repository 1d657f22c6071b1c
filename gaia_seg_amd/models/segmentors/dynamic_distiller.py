"""DynamicDistiller — a frozen teacher segmentor over the sampled student.

Host-side mirror of gaiaseg/models/segmentors/dynamic_distiller.py:152-413, quirks included: the
student's decode-head losses come without the 'decode.' prefix, both logit maps are resized with the
STUDENT's align_corners, the logit loss has no T^2 factor, and the pairwise loss is taken on the
single column the reference's slice selects (:329-330).  The two distillation losses run on the HIP
kernels of csrc/distill.hip (models/losses/distill_loss.py).  Not in the reference: the opt-in
channel-wise distillation loss ``channel_loss_seg`` of csrc/cwd.hip on the two low-resolution logit maps
(DESIGN.md section 24), the structural term the one-column pairwise loss does not provide.

Deliberate deviation: the teacher is held OUTSIDE module registration.  It is
absent from parameters(), modules(), state_dict() and active_parameters(), so the parameter arena,
the gradient reducer, the optimizer groups, wrap_fp16_model and the finetune snapshot never see it,
and a checkpoint holds the student alone under the keys of a DynamicEncoderDecoder (mmcv would save
'teacher_segmentor.*' too; core/checkpoint.py drops such keys when it meets them).
"""
import numpy as np  # noqa: F401  (the window is drawn from numpy's global state: losses/distill_loss.py)
import torch

from ...hip import ops, streams
from ..builder import SEGMENTORS, build_segmentor
from ..losses.distill_loss import (channel_distill_loss, draw_pairwise_window, pairwise_loss,
                                   teacher_distill_loss)
from .dynamic_encoder_decoder import DynamicEncoderDecoder

@SEGMENTORS.register_module()
class DynamicDistiller(DynamicEncoderDecoder):
    # the host draws a pairwise window every step: a step is never captured into a step graph
    step_graph_capturable = False
    fixed_teacher = True

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, teacher_segmentor=None,
                 train_cfg=None, test_cfg=None, pretrained=None, teacher_ckpt=None,
                 has_distill_loss=True, distill_loss_temperature=1, has_pairwise_loss=True,
                 pairwise_loss_temperature=1, distill_loss_weight=1, pairwise_loss_weight=1,
                 has_channel_loss=False, channel_loss_temperature=1, channel_loss_weight=1):
        if isinstance(decode_head, (list, tuple)):
            raise ValueError("DynamicDistiller: a cascade of decode heads is not supported: the distillation "
                             "losses compare ONE student logit map with the teacher's")
        super().__init__(backbone=backbone, decode_head=decode_head, neck=neck,
                         auxiliary_head=auxiliary_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained)
        self.has_distill_loss = bool(has_distill_loss)
        self.has_pairwise_loss = bool(has_pairwise_loss)
        self.distill_loss_temperature = distill_loss_temperature
        self.distill_loss_weight = distill_loss_weight
        self.pairwise_loss_temperature = pairwise_loss_temperature
        self.pairwise_loss_weight = pairwise_loss_weight
        self.has_channel_loss = bool(has_channel_loss)
        self.channel_loss_temperature = channel_loss_temperature
        self.channel_loss_weight = channel_loss_weight
        teacher = None
        # (:190-206; all off: "debug mode")
        if self.has_distill_loss or self.has_pairwise_loss or self.has_channel_loss:
            if teacher_segmentor is None:
                raise ValueError("DynamicDistiller: teacher_segmentor (the teacher's model config) is "
                                 "missing")
            teacher = build_segmentor(teacher_segmentor, test_cfg=test_cfg)
            assert teacher_ckpt is not None, "Teacher ckpt is missed !"
            if teacher.num_classes != self.num_classes:
                raise ValueError("DynamicDistiller: the teacher predicts %d classes, the student %d"
                                 % (teacher.num_classes, self.num_classes))
            from ...core.checkpoint import load_checkpoint
            load_checkpoint(teacher, teacher_ckpt, map_location="cpu")   # a local file, no URLs
            teacher.eval()
            for p in teacher.parameters():
                p.requires_grad_(False)
        # past nn.Module.__setattr__: not a registered child
        object.__setattr__(self, "teacher_segmentor", teacher)

    def _apply(self, fn, *args, **kwargs):
        """.to() / .cuda() / .float() carry the unregistered teacher along."""
        super()._apply(fn, *args, **kwargs)
        if self.teacher_segmentor is not None:
            self.teacher_segmentor._apply(fn, *args, **kwargs)
        return self

    def prepare_distill_feature(self, img, img_metas):
        """(:264-274) the teacher's feature maps and its LOW-resolution logits: the resize to the image
        size happens inside the loss kernel.  No tape, fp32 convolutions whatever the step's precision."""
        t = self.teacher_segmentor
        # (the branch-pattern traces of the parity tests describe the student alone)
        traces = ops.RELU_TRACE, ops.POOL_TRACE
        ops.RELU_TRACE = ops.POOL_TRACE = None
        try:
            with torch.no_grad(), ops.train_precision("fp32"), ops.forward_precision("fp32"):
                x = t.extract_feat(img)
                out = t._decode_head_forward_test(x, img_metas)
        finally:
            ops.RELU_TRACE, ops.POOL_TRACE = traces
        return x, out

    def forward_train(self, img, img_metas, gt_semantic_seg):
        """(:370-413)"""
        distill = ((self.has_distill_loss or self.has_pairwise_loss or self.has_channel_loss)
                   and self.teacher_segmentor is not None)
        if distill:
            teacher_x, teacher_logits = self.prepare_distill_feature(img, img_metas)
        x = self.extract_feat(img)
        dev = img.device
        branch = self.with_auxiliary_head and ops.BRANCH_AUX and dev.type == "cuda"
        if branch:   # the auxiliary head(s) beside the decode head, as in EncoderDecoder.forward_train
            streams.prefork_branch(dev, streams.SLOT_AUX)
        seg_logits = self.decode_head.forward(x)
        losses = self.decode_head.losses(seg_logits, gt_semantic_seg)
        if distill and self.has_distill_loss:
            losses["distill_loss_seg"] = teacher_distill_loss(
                seg_logits, teacher_logits, img.shape[2:], T=self.distill_loss_temperature,
                weight=self.distill_loss_weight, align_corners=self.align_corners)
        if distill and self.has_pairwise_loss:
            feat = x[-1]
            window = draw_pairwise_window(feat.shape[2], feat.shape[3])
            losses["pairwise_loss_seg"] = pairwise_loss(
                feat, teacher_x[-1], window, T=self.pairwise_loss_temperature,
                weight=self.pairwise_loss_weight)
        if distill and self.has_channel_loss:
            # at logit resolution: a teacher at another output stride is refused (ValueError, both shapes)
            losses["channel_loss_seg"] = channel_distill_loss(
                seg_logits, teacher_logits, T=self.channel_loss_temperature,
                weight=self.channel_loss_weight)
        if self.with_auxiliary_head:
            with streams.branch_scope(dev, branch, forked=True):
                loss_aux = self._auxiliary_head_forward_train(x, img_metas, gt_semantic_seg)
            if branch:
                streams.join_branch(dev, streams.SLOT_AUX)
            losses.update(loss_aux)
        return losses
