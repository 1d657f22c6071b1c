"""In-place distillation loss of the sandwich rule, computed by the fused HIP kernels of csrc/distill.hip.

Reference: the distillation branch of the decode heads' forward_train
(gaiaseg/models/decode_heads/dynamic_psp_head.py:176-245, dynamic_fcn_head.py:161-231):
    loss_seg = distillation_weight * mean_n( sum_{c,h,w} -softmax(t/T) * log softmax(s/T) ) / D
with D = 1000 (PSP head) or 2000 (FCN head), optionally after resizing both logits to the label size.
No ground-truth term; the teacher (the MAX subnet's logits of the same iteration) gets no gradient.
"""
import ctypes

import torch

from ...hip import lib as _lib
from ...hip.runtime import WORKSPACE, current_stream_ptr, require_gpu_tensor, round_up

# the reference's defaults (dynamic_psp_head.py:196-200)
KD_DEFAULTS = dict(T=2.0, distillation_weight=0.5, interpolation=False)


def kd_desc(student, teacher, out_hw, T, align_corners, interpolation):
    n, c, h, w = student.shape
    if tuple(teacher.shape) != (n, c, h, w):
        raise ValueError("student logits %s and teacher logits %s differ in shape"
                         % (tuple(student.shape), tuple(teacher.shape)))
    d = _lib.KdDesc()
    d.N, d.h, d.w, d.Cls = n, h, w, c
    d.H, d.W = (int(out_hw[0]), int(out_hw[1])) if interpolation else (h, w)
    d.s_sn, d.s_sc, d.s_sh, d.s_sw = student.stride()
    d.t_sn, d.t_sc, d.t_sh, d.t_sw = teacher.stride()
    d.T = float(T)
    d.align_corners = 1 if align_corners else 0
    d.interpolation = 1 if interpolation else 0
    return d


class _FusedKD(torch.autograd.Function):
    """scale * sum_{n,c,Y,X} -softmax(t/T) log softmax(s/T) as one fp32 scalar; gradient to the
    student's low-resolution logits only."""

    @staticmethod
    def forward(ctx, student, teacher, out_hw, T, align_corners, interpolation, scale):
        require_gpu_tensor(student, "seg_logit")
        require_gpu_tensor(teacher, "teacher_logits")
        L = _lib.load()
        dev = student.device
        d = kd_desc(student, teacher, out_hw, T, align_corners, interpolation)
        lse_s = torch.empty((d.N, d.H, d.W), dtype=torch.float32, device=dev)
        lse_t = torch.empty_like(lse_s)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = WORKSPACE.get(L.gs_kd_workspace_bytes(ctypes.byref(d)), dev)
        _lib.check(L.gs_kd_forward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                   lse_s.data_ptr(), lse_t.data_ptr(), float(scale), out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), current_stream_ptr()), "gs_kd_forward")
        ctx.desc, ctx.scale = d, float(scale)
        ctx.save_for_backward(student, teacher, lse_s, lse_t)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from ...hip import ops as _ops
        prev_slot = _ops.adopt_current_stream()   # (the auxiliary head's loss runs on the branch stream)
        try:
            student, teacher, lse_s, lse_t = ctx.saved_tensors
            L = _lib.load()
            d = ctx.desc
            n, c, h, w = student.shape
            ld = round_up(c, 4)
            buf = torch.empty((n, h, w, ld), dtype=torch.float32, device=student.device)
            ws = WORKSPACE.get(L.gs_kd_backward_workspace_bytes(ctypes.byref(d), ld), student.device)
            _lib.check(L.gs_kd_backward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                        lse_s.data_ptr(), lse_t.data_ptr(), ctx.scale, buf.data_ptr(),
                                        ld, ws.data_ptr(), ws.numel(), current_stream_ptr()),
                       "gs_kd_backward")
            buf.mul_(grad_loss)   # the upstream scalar, on the device (no host sync)
            return buf[..., :c].permute(0, 3, 1, 2), None, None, None, None, None, None
        finally:
            _ops.restore_stream_slot(prev_slot)


def kd_loss(student, teacher, label_hw, T=2.0, distillation_weight=0.5, divisor=1000.0,
            interpolation=False, align_corners=False):
    """The reference's distillation loss_seg (see the module docstring); ``teacher`` is detached."""
    n = student.shape[0]
    scale = float(distillation_weight) / (n * float(divisor))
    return _FusedKD.apply(student, teacher.detach(), tuple(int(v) for v in label_hw), float(T),
                          bool(align_corners), bool(interpolation), scale)
