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
from ...hip.streams import adopt_current_stream

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
        with adopt_current_stream():   # (the auxiliary head's loss runs on the branch stream)
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


def kd_loss(student, teacher, label_hw, T=2.0, distillation_weight=0.5, divisor=1000.0,
            interpolation=False, align_corners=False):
    """The reference's distillation loss_seg (see the module docstring); ``teacher`` is detached."""
    n = student.shape[0]
    scale = float(distillation_weight) / (n * float(divisor))
    return _FusedKD.apply(student, teacher.detach(), tuple(int(v) for v in label_hw), float(T),
                          bool(align_corners), bool(interpolation), scale)


# ---- fixed-teacher distillation (DynamicDistiller; gaiaseg/models/segmentors/dynamic_distiller.py) ----
def distill_desc(student, teacher, out_hw, T, align_corners):
    n, c, hs, ws = student.shape
    if teacher.dim() != 4 or teacher.shape[0] != n or teacher.shape[1] != c:
        raise ValueError("student logits %s and teacher logits %s differ in batch or class count"
                         % (tuple(student.shape), tuple(teacher.shape)))
    d = _lib.DistillDesc()
    d.N, d.Cls, d.hs, d.ws = n, c, hs, ws
    d.ht, d.wt = int(teacher.shape[2]), int(teacher.shape[3])
    d.H, d.W = int(out_hw[0]), int(out_hw[1])
    d.s_sn, d.s_sc, d.s_sh, d.s_sw = student.stride()
    d.t_sn, d.t_sc, d.t_sh, d.t_sw = teacher.stride()
    d.T = float(T)
    d.align_corners = 1 if align_corners else 0
    return d


class _TeacherDistill(torch.autograd.Function):
    """scale * sum_{n,c,Y,X} -softmax(t'/T) log softmax(s'/T), s' and t' the two logit maps resized to
    ``out_hw`` inside the kernel (each from its own resolution); gradient to the student's logits."""

    @staticmethod
    def forward(ctx, student, teacher, out_hw, T, align_corners, scale):
        require_gpu_tensor(student, "seg_logit")
        require_gpu_tensor(teacher, "teacher_logits")
        L = _lib.load()
        dev = student.device
        d = distill_desc(student, teacher, out_hw, T, align_corners)
        lse_s = torch.empty((d.N, d.H, d.W), dtype=torch.float32, device=dev)
        lse_t = torch.empty_like(lse_s)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = WORKSPACE.get(L.gs_distill_workspace_bytes(ctypes.byref(d)), dev)
        _lib.check(L.gs_distill_forward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                        lse_s.data_ptr(), lse_t.data_ptr(), float(scale),
                                        out.data_ptr(), ws.data_ptr(), ws.numel(),
                                        current_stream_ptr()), "gs_distill_forward")
        ctx.desc, ctx.scale = d, float(scale)
        ctx.save_for_backward(student, teacher, lse_s, lse_t)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        with adopt_current_stream():
            student, teacher, lse_s, lse_t = ctx.saved_tensors
            L = _lib.load()
            d = ctx.desc
            n, c, h, w = student.shape
            ld = round_up(c, 4)
            buf = torch.empty((n, h, w, ld), dtype=torch.float32, device=student.device)
            ws = WORKSPACE.get(L.gs_distill_backward_workspace_bytes(ctypes.byref(d), ld),
                               student.device)
            _lib.check(L.gs_distill_backward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                             lse_s.data_ptr(), lse_t.data_ptr(), ctx.scale,
                                             buf.data_ptr(), ld, ws.data_ptr(), ws.numel(),
                                             current_stream_ptr()), "gs_distill_backward")
            buf.mul_(grad_loss)   # the upstream scalar, on the device (no host sync)
            return buf[..., :c].permute(0, 3, 1, 2), None, None, None, None, None


def teacher_distill_loss(student, teacher, out_hw, T=1, weight=1, align_corners=False):
    """distill_loss of the reference's DynamicDistiller (:341-356 behind the two resizes of :269-273 and
    :398-402): weight * sum -softmax(t'/T) log_softmax(s'/T) / (N * H * W) at the image size ``out_hw``;
    no T^2 factor; ``teacher`` is detached and may have another resolution than ``student``."""
    h, w = int(out_hw[0]), int(out_hw[1])
    scale = float(weight) / (student.shape[0] * h * w)
    return _TeacherDistill.apply(student, teacher.detach(), (h, w), float(T), bool(align_corners), scale)


def draw_pairwise_window(H, W):
    """The reference's window (dynamic_distiller.py:323-330), drawn from numpy's GLOBAL state (h first,
    then w) so that set_random_seed reproduces it: rows start_h .. start_h + step_h of the single
    column start_w + step_w -- the slice as the reference writes it.  (y0, y1, x0, x1, step_h, step_w)."""
    import numpy as np
    step_h = int(0.5 * H)
    step_w = int(0.5 * W)
    choice_h = np.random.uniform(0, 0.5)
    choice_w = np.random.uniform(0, 0.5)
    start_h = int(choice_h * H)
    start_w = int(choice_w * W)
    col = start_w + step_w
    return (start_h, start_h + step_h, col, col + 1, step_h, step_w)


def pairwise_desc(student, teacher, window, T):
    n, cs, h, w = student.shape
    if teacher.dim() != 4 or teacher.shape[0] != n:
        raise ValueError("student features %s and teacher features %s differ in batch size"
                         % (tuple(student.shape), tuple(teacher.shape)))
    y0, y1, x0, x1 = (int(v) for v in window[:4])
    ht, wt = int(teacher.shape[2]), int(teacher.shape[3])
    if not (0 <= y0 < y1 <= min(h, ht) and 0 <= x0 < x1 <= min(w, wt)):
        raise ValueError("pairwise window rows %d:%d, columns %d:%d is empty or leaves the student "
                         "(%dx%d) or teacher (%dx%d) feature map" % (y0, y1, x0, x1, h, w, ht, wt))
    d = _lib.PairwiseDesc()
    d.N, d.Cs, d.Ct, d.H, d.W, d.Ht, d.Wt = n, cs, int(teacher.shape[1]), h, w, ht, wt
    d.y0, d.y1, d.x0, d.x1 = y0, y1, x0, x1
    d.s_sn, d.s_sc, d.s_sh, d.s_sw = student.stride()
    d.t_sn, d.t_sc, d.t_sh, d.t_sw = teacher.stride()
    d.T = float(T)
    return d


class _Pairwise(torch.autograd.Function):
    """The pairwise affinity loss on a window (gs_pairwise_*); gradient to the student map only."""

    @staticmethod
    def forward(ctx, student, teacher, window, T, scale):
        require_gpu_tensor(student, "student feature map")
        require_gpu_tensor(teacher, "teacher feature map")
        L = _lib.load()
        d = pairwise_desc(student, teacher, window, T)
        nbytes = L.gs_pairwise_save_bytes(ctypes.byref(d))
        if nbytes == 0:
            _lib.check(-1, "gs_pairwise_forward (window of %d pixels; at most %d)"
                       % ((d.y1 - d.y0) * (d.x1 - d.x0), _lib.PAIRWISE_MAX_P))
        save = torch.empty(round_up(nbytes, 8) // 8, dtype=torch.float64, device=student.device)
        out = torch.empty(1, dtype=torch.float32, device=student.device)
        _lib.check(L.gs_pairwise_forward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                         float(scale), out.data_ptr(), save.data_ptr(),
                                         save.numel() * 8, current_stream_ptr()),
                   "gs_pairwise_forward")
        ctx.desc, ctx.scale = d, float(scale)
        ctx.save_for_backward(student, save)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        with adopt_current_stream():
            student, save = ctx.saved_tensors
            L = _lib.load()
            d = ctx.desc
            n, c, h, w = student.shape
            ld = round_up(c, 4)
            buf = torch.empty((n, h, w, ld), dtype=torch.float32, device=student.device)
            _lib.check(L.gs_pairwise_backward(ctypes.byref(d), student.data_ptr(), save.data_ptr(),
                                              save.numel() * 8, ctx.scale, buf.data_ptr(), ld,
                                              current_stream_ptr()), "gs_pairwise_backward")
            buf.mul_(grad_loss)   # the upstream scalar, on the device (no host sync)
            return buf[..., :c].permute(0, 3, 1, 2), None, None, None, None


def pairwise_loss(student_feat, teacher_feat, window, T=1, weight=1):
    """pairwise_loss of the reference's DynamicDistiller (:309-339) on ``window`` = (y0, y1, x0, x1,
    step_h, step_w) as draw_pairwise_window returns it: the divisor is N * step_h * step_w although the
    window is one column.  ``teacher_feat`` is detached; channel counts may differ."""
    step_h, step_w = int(window[4]), int(window[5])
    scale = float(weight) / (student_feat.shape[0] * step_h * step_w)
    return _Pairwise.apply(student_feat, teacher_feat.detach(), tuple(int(v) for v in window[:4]),
                           float(T), scale)


# ---- channel-wise distillation (Shu et al., ICCV 2021; mmrazor's ChannelWiseDivergence) ----
def _cwd_check_shapes(student, teacher):
    if student.dim() != 4 or tuple(teacher.shape) != tuple(student.shape):
        raise ValueError("channel-wise distillation needs student logits %s and teacher logits %s of one "
                         "shape (a teacher at another output stride is not supported)"
                         % (tuple(student.shape), tuple(teacher.shape)))


def cwd_desc(student, teacher, T):
    _cwd_check_shapes(student, teacher)
    d = _lib.CwdDesc()
    d.N, d.C, d.H, d.W = student.shape
    d.s_sn, d.s_sc, d.s_sh, d.s_sw = student.stride()
    d.t_sn, d.t_sc, d.t_sh, d.t_sw = teacher.stride()
    d.T = float(T)
    return d


class _ChannelDistill(torch.autograd.Function):
    """scale * T^2 * sum_{n,c} KL(softmax_pixels(t/T) || softmax_pixels(s/T)) as one fp32 scalar
    (gs_cwd_*); gradient to the student's logits only."""

    @staticmethod
    def forward(ctx, student, teacher, T, scale):
        require_gpu_tensor(student, "seg_logit")
        require_gpu_tensor(teacher, "teacher_logits")
        L = _lib.load()
        dev = student.device
        d = cwd_desc(student, teacher, T)
        lse_s = torch.empty((d.N, d.C), dtype=torch.float32, device=dev)
        lse_t = torch.empty_like(lse_s)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        ws = WORKSPACE.get(L.gs_cwd_workspace_bytes(ctypes.byref(d)), dev)
        _lib.check(L.gs_cwd_forward(ctypes.byref(d), student.data_ptr(), teacher.data_ptr(),
                                    lse_s.data_ptr(), lse_t.data_ptr(), float(scale), out.data_ptr(),
                                    ws.data_ptr(), ws.numel(), current_stream_ptr()), "gs_cwd_forward")
        ctx.desc, ctx.scale = d, float(scale)
        ctx.save_for_backward(student, teacher, lse_s, lse_t)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        with adopt_current_stream():
            student, teacher, lse_s, lse_t = ctx.saved_tensors
            L = _lib.load()
            n, c, h, w = student.shape
            ld = round_up(c, 4)
            buf = torch.empty((n, h, w, ld), dtype=torch.float32, device=student.device)
            _lib.check(L.gs_cwd_backward(ctypes.byref(ctx.desc), student.data_ptr(), teacher.data_ptr(),
                                         lse_s.data_ptr(), lse_t.data_ptr(), ctx.scale, buf.data_ptr(),
                                         ld, current_stream_ptr()), "gs_cwd_backward")
            buf.mul_(grad_loss)   # the upstream scalar, on the device (no host sync)
            return buf[..., :c].permute(0, 3, 1, 2), None, None, None


def channel_distill_loss(student, teacher, T=1, weight=1):
    """Channel-wise distillation of two logit maps of one shape [N, C, H, W]: every class map becomes a
    distribution over its H * W pixels (softmax of x / T), and the loss is
    weight * T^2 / (N * C) * sum_{n,c} KL(phi(teacher) || phi(student)) -- mmrazor's
    ChannelWiseDivergence.  No labels, no resize; ``teacher`` is detached."""
    require_gpu_tensor(student, "seg_logit")
    require_gpu_tensor(teacher, "teacher_logits")
    _cwd_check_shapes(student, teacher)
    scale = float(weight) / (student.shape[0] * student.shape[1])
    return _ChannelDistill.apply(student, teacher.detach(), float(T), scale)
