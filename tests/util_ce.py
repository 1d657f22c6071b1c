"""Cases, inputs and the float64 CPU reference for the fused resize + cross-entropy kernels
(csrc/loss.hip), the host-side routing of gs_ce_backward_ws restated in Python, and the guarded C-ABI
calls that tests/test_ce_loss_gpu.py and its GS_CE_ROWCLS child process (``python tests/util_ce.py``,
see main()) share.

The reference is plain torch: F.interpolate(bilinear) + F.cross_entropy(reduction="none") times the pixel
weight, summed; its gradient comes from autograd."""
import collections
import ctypes
import functools
import os
import sys

import torch
import torch.nn.functional as F

TCH, CCH = 20, 32   # classes per pass of the tile kernels / of the gather kernel (csrc/loss.hip)

# route = (form gs_ce_backward_ws takes with a workspace, its block size, block size of gs_ce_backward)
Case = collections.namedtuple("Case", "name shape size align ignore seed tie route")

# logits (N, Cls, h, w) -> labels (H, W).  The smallest shapes that reach each launch; test_ce_loss.py
# asserts the route of every row from the three host predicates below, and that each seed keeps every
# pixel's float64 top-2 gap above 1e-4.
#   * pow2 tile form at 64 / 128 / 256 threads: pow2-4x4, pow2-16x32, pow2-32x32-h1w1.
#   * gather form (ce_bwd_kernel) at 64 / 128 / 256 threads through gs_ce_backward and workspace = NULL on
#     EVERY case; the only form of the three gather-* cases.  128 threads: pow2-4x4 (and ignore-in-range,
#     tie), whose support (2 * 4 + 1)^2 = 81 lies in (64, 128] -- the same 9 x 9 as (2,19,5,7) -> (20,28),
#     so that shape is not added.
#   * row-tile form: ce_bwd_rowtile_kernel<5> here, <10> and <4> in the GS_CE_ROWCLS child on the same rows.
#   * rowtile-64px-dead: the shape (1,45,2,3) -> (16,24) first proposed for this row is 8 x 8, a power of
#     two, and takes the pow2 tile form; (12,32) keeps h * w = 6, 12 tiles (4 dead row groups of 16), 45
#     classes (three class passes) and H * W = 384 = 64 * 6 exactly on the row-tile threshold, at the
#     ratios 6 x 10.67.
#   * gather-1x1-align has ONE label pixel; it keeps a valid label (no ignored row, no out-of-range labels:
#     there is no room for them), else its gradient would be all zero.
CASES = [
    Case("pow2-4x4", (2, 19, 4, 4), (16, 16), False, 255, 2, False, ("pow2", 64, 128)),
    # sy = 16 != sx = 32, 512 pixels per tile
    Case("pow2-16x32", (1, 19, 2, 2), (32, 64), False, 255, 1, False, ("pow2", 128, 256)),
    # 1024 pixels per tile, h = w = 1 (i1 == i0 everywhere), Cls = TCH + 1: a second class pass of one class
    Case("pow2-32x32-h1w1", (1, 21, 1, 1), (32, 32), False, 255, 1, False, ("pow2", 256, 256)),
    Case("pow2-2x2-cls20", (1, 20, 2, 3), (4, 6), False, 255, 1, False, ("pow2", 64, 64)),          # Cls == TCH
    Case("rowtile-38px", (2, 19, 5, 7), (33, 41), False, 255, 5, False, ("rowtile", 256, 256)),    # 3 passes / lane
    Case("rowtile-64px-dead", (1, 45, 2, 3), (12, 32), False, 255, 1, False, ("rowtile", 256, 256)),
    Case("rowtile-1to1", (1, 19, 6, 5), (6, 5), False, 255, 1, False, ("rowtile", 256, 64)),
    Case("rowtile-align", (2, 19, 9, 6), (10, 47), True, 255, 2, False, ("rowtile", 256, 64)),      # one-row tiles
    Case("rowtile-align-h1", (1, 19, 1, 3), (5, 9), True, 255, 1, False, ("rowtile", 256, 128)),   # sh == 0
    Case("rowtile-cls1", (1, 1, 3, 3), (7, 5), False, 255, 1, False, ("rowtile", 256, 64)),        # all exactly 0
    # ratio 17.5 x 16.3 > 64 pixels per tile, not a power of two; Cls == CCH + 1
    Case("gather-big", (1, 33, 2, 3), (35, 49), False, 255, 1, False, ("gather", 256, 256)),
    Case("gather-down", (1, 19, 9, 6), (4, 3), False, 255, 1, False, ("gather", 64, 64)),           # down-scaling
    Case("gather-1x1-align", (1, 19, 4, 4), (1, 1), True, 255, 1, False, ("gather", 64, 64)),       # scale == 0
    Case("rowtile-cls150", (1, 150, 3, 4), (13, 9), False, 255, 2, False, ("rowtile", 256, 64)),
    Case("ignore-in-range", (2, 19, 4, 4), (16, 16), False, 3, 2, False, ("pow2", 64, 128)),
    Case("ignore-minus100", (1, 19, 3, 4), (13, 9), False, -100, 1, False, ("rowtile", 256, 64)),
    # channels 2 and 7 identical (and raised, so that they are the maximum at many pixels): argmax is 2
    Case("tie", (1, 19, 3, 4), (12, 16), False, 255, 2, True, ("pow2", 64, 128)),
]
CASE_IDS = [c.name for c in CASES]
TIE_LO, TIE_HI = 2, 7
ROWTILE_CASES = [c for c in CASES if c.route[0] == "rowtile"]


def round_up(x, m):
    return (x + m - 1) // m * m


# ---- gs_ce_backward_ws's host-side dispatch, restated -------------------------------------------------------
def pow2_scales(shape, size, align):
    """ce_tile_scales: (sy, sx) for a power-of-two integer up-scaling without align_corners, else None"""
    (_, _, h, w), (hh, ww) = shape, size
    if align or hh % h or ww % w:
        return None
    sy, sx = hh // h, ww // w
    ok = all(v >= 2 and v & (v - 1) == 0 for v in (sy, sx))
    return (sy, sx) if ok else None


def rowtile_ok(shape, size):
    """ce_rowtile_ok: an up-scaling of at most 64 label pixels per logit pixel"""
    (_, _, h, w), (hh, ww) = shape, size
    return hh >= h and ww >= w and hh * ww <= 64 * h * w


def gather_threads(shape, size):
    """gs_ce_backward's block size from the support of one logit pixel"""
    (_, _, h, w), (hh, ww) = shape, size
    sup = (2 * hh // h + 1) * (2 * ww // w + 1)
    return 256 if sup > 128 else 128 if sup > 64 else 64


def route(shape, size, align):
    s = pow2_scales(shape, size, align)
    if s is not None:
        px = s[0] * s[1]
        return "pow2", (256 if px >= 1024 else 128 if px >= 512 else 64), gather_threads(shape, size)
    if rowtile_ok(shape, size):
        return "rowtile", 256, gather_threads(shape, size)
    t = gather_threads(shape, size)
    return "gather", t, t


def backward_workspace_bytes(shape, size, align, ld_d):
    n, _, h, w = shape
    return 0 if route(shape, size, align)[0] == "gather" else n * (h + 1) * (w + 1) * 4 * ld_d * 4


# ---- inputs -----------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "logits labels pixel_weight class_weight bad_pixels")


@functools.lru_cache(maxsize=None)
def ce_inputs(name):
    """seeded randn * 3 logits; labels uniform in [0, Cls) with the first row and a small block ignored and
    three pixels out of range (-1, Cls, 1 << 40); pixel_weight (rand > 0.3), class_weight rand + 0.5"""
    case = CASES[CASE_IDS.index(name)]
    (n, cls, h, w), (hh, ww) = case.shape, case.size
    g = torch.Generator().manual_seed(case.seed)
    logits = torch.randn(n, cls, h, w, generator=g) * 3
    if case.tie:
        logits[:, TIE_LO] += 3.0
        logits[:, TIE_HI] = logits[:, TIE_LO]
    labels = torch.randint(0, cls, (n, hh, ww), generator=g)
    bad = []
    if hh * ww > 1:
        labels[:, 0, :] = case.ignore
        labels[0, 1:1 + max(1, hh // 4), 1:1 + max(1, ww // 4)] = case.ignore
        bad = [((n - 1, hh - 1, ww - 1), -1), ((n - 1, hh - 1, 0), cls), ((0, hh // 2, ww - 1), 1 << 40)]
        for pos, val in bad:
            labels[pos] = val
    pw = (torch.rand(n, hh, ww, generator=g) > 0.3).float()
    cw = torch.rand(cls, generator=g) + 0.5
    return Inputs(logits, labels, pw, cw, tuple(p for p, _ in bad))


def valid_mask(case, labels):
    return (labels != case.ignore) & (labels >= 0) & (labels < case.shape[1])


# ---- reference --------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "loss correct lse dlogits prob softmax argmax gap")


def lowest_argmax(up):
    """argmax over dim 1 with the kernels' rule written out: a strict `>` scan keeps the LOWEST index of the
    maximum (torch.argmax promises no order among ties)"""
    cls = up.shape[1]
    idx = torch.arange(cls).view(1, cls, 1, 1).expand_as(up)
    top = up.max(dim=1, keepdim=True).values
    return torch.where(up == top, idx, torch.full_like(idx, cls)).min(dim=1).values


def ce_formula(case, inp, weighted, dtype):
    """loss sum, #(argmax == raw label), lse [N,H,W], dlogits [N,h,w,Cls] for grad_scale = 1 (it is linear in
    grad_scale), softmax(resized)[label] with 2.0 at invalid pixels, softmax [N,H,W,Cls], argmax, and the
    smallest top-2 gap of the resized logits (the tie case: without the duplicate channel)"""
    cls = case.shape[1]
    x = inp.logits.detach().to(dtype).clone().requires_grad_(True)
    up = F.interpolate(x, size=case.size, mode="bilinear", align_corners=case.align)
    valid = valid_mask(case, inp.labels)
    lab = torch.where(valid, inp.labels, torch.full_like(inp.labels, case.ignore))
    cw = inp.class_weight.to(dtype) if weighted else None
    loss = F.cross_entropy(up, lab, weight=cw, reduction="none", ignore_index=case.ignore)
    if weighted:
        loss = loss * inp.pixel_weight.to(dtype)
    total = loss.sum()
    total.backward()
    up = up.detach()
    soft = up.softmax(dim=1)
    amax = lowest_argmax(up)
    prob = soft.gather(1, torch.where(valid, lab, torch.zeros_like(lab)).unsqueeze(1)).squeeze(1)
    prob = torch.where(valid, prob, torch.full_like(prob, 2.0))
    ranked = up if not case.tie else up[:, [c for c in range(cls) if c != TIE_HI]]
    gap = float("inf")
    if ranked.shape[1] > 1:
        top2 = ranked.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
    return Ref(float(total.detach()), int((amax == inp.labels).sum()), torch.logsumexp(up, dim=1),
               x.grad.permute(0, 2, 3, 1).contiguous(), prob, soft.permute(0, 2, 3, 1).contiguous(), amax, gap)


@functools.lru_cache(maxsize=None)
def ce_ref(name, weighted):
    """the float64 reference of a case, computed once and shared (do not modify)"""
    return ce_formula(CASES[CASE_IDS.index(name)], ce_inputs(name), weighted, torch.float64)


# ---- the guarded C-ABI calls (GPU) ----------------------------------------------------------------------------
DEV = "cuda"
TOL = 5e-5           # this operator's bound in the suite (tests/test_hip_ops_gpu.py)
LOSS_TOL = 2e-5      # * max(1, |ref|): test_fused_resize_ce_fwd_bwd's bound
SENTINEL = 7.0
TAIL = 16
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
LOGIT_PAD = 5
LAYOUTS = ("nhwc-padded", "nchw")
FORMS = ("ws", "null", "direct")


def stream():
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    return current_stream_ptr()


class Workspace:
    """exactly ``need`` bytes of 0xFF (NaN as floats and doubles) in front of a guard"""

    def __init__(self, need):
        assert need > 0
        self.need = need
        self.buf = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
        self.buf[:need] = 0xFF
        self.buf[need:] = GUARD_BYTE

    def ptr(self):
        return self.buf.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.need:] == GUARD_BYTE).all()), "the workspace was overrun"


class Out:
    """``numel`` elements of the sentinel, followed by a sentinel tail"""

    def __init__(self, numel, dtype=torch.float32, fill=SENTINEL):
        self.numel, self.fill = numel, fill
        self.buf = torch.full((numel + TAIL,), fill, dtype=dtype, device=DEV)

    def ptr(self):
        return self.buf.data_ptr()

    def get(self, what):
        """synchronise; the tail is untouched; the written part on the CPU, free of NaN"""
        torch.cuda.synchronize()
        out = self.buf.cpu()
        assert bool((out[self.numel:] == self.fill).all()), "%s: a store past the end" % what
        got = out[:self.numel]
        if got.is_floating_point():
            assert bool(torch.isfinite(got).all()), "%s: NaN -- a pad column or unwritten scratch was read" % what
        return got

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == self.fill).all())


class Operands:
    """a case's inputs on the device in one logits layout, and its descriptor"""

    def __init__(self, case, layout, weighted):
        from gaia_seg_amd.hip import lib
        inp = ce_inputs(case.name)
        n, cls, h, w = case.shape
        self.case, self.numel = case, inp.labels.numel()
        if layout == "nhwc-padded":   # channel pitch Cls + 5, NaN in the pad columns
            ld = cls + LOGIT_PAD
            buf = torch.full((n, h, w, ld), float("nan"))
            buf[..., :cls] = inp.logits.permute(0, 2, 3, 1)
            strides = (h * w * ld, w * ld, ld, 1)
        else:
            assert layout == "nchw"
            buf = inp.logits.contiguous()
            strides = (cls * h * w, w, 1, h * w)
        self.logits = buf.to(DEV)
        self.labels = inp.labels.to(DEV)
        self.pw = inp.pixel_weight.to(DEV) if weighted else None
        self.cw = inp.class_weight.to(DEV) if weighted else None
        d = lib.CeDesc()
        d.N, d.h, d.w, d.Cls = n, h, w, cls
        d.H, d.W = case.size
        d.l_sn, d.l_sh, d.l_sw, d.l_sc = strides
        d.ignore_index, d.align_corners = case.ignore, int(case.align)
        self.desc = d

    def db(self):
        return ctypes.byref(self.desc)

    def pw_ptr(self):
        return self.pw.data_ptr() if self.pw is not None else None

    def cw_ptr(self):
        return self.cw.data_ptr() if self.cw is not None else None


def run_forward(L, op, with_lse=True, scales=None):
    """gs_ce_forward (scales None) -> (out [2] float64, lse [N,H,W] or None); gs_ce_forward_scaled
    (scales = (loss_scale, acc_scale)) -> (out2 [2] float32, lse)"""
    from gaia_seg_amd.hip import lib
    case = op.case
    ws = Workspace(L.gs_ce_workspace_bytes(op.db()))
    lse = Out(op.numel) if with_lse else None
    out = Out(2, torch.float64 if scales is None else torch.float32)
    lse_ptr = lse.ptr() if with_lse else None
    if scales is None:
        rc = L.gs_ce_forward(op.db(), op.logits.data_ptr(), op.labels.data_ptr(), op.pw_ptr(), op.cw_ptr(),
                             lse_ptr, out.ptr(), ws.ptr(), ws.need, stream())
    else:
        rc = L.gs_ce_forward_scaled(op.db(), op.logits.data_ptr(), op.labels.data_ptr(), op.pw_ptr(), op.cw_ptr(),
                                    lse_ptr, scales[0], scales[1], out.ptr(), ws.ptr(), ws.need, stream())
    lib.check(rc, "gs_ce_forward")
    ws.check()
    got = out.get("out")
    return got, (lse.get("lse").view(case.shape[0], *case.size) if with_lse else None)


def run_backward(L, op, lse_dev, form, ld_d, grad_scale):
    """one of FORMS -> dlogits [N,h,w,Cls]; the pad columns Cls..ld_d-1 are exactly 0.0, the tail and the
    workspace guard untouched"""
    from gaia_seg_amd.hip import lib
    n, cls, h, w = op.case.shape
    dl = Out(n * h * w * ld_d)
    head = (op.db(), op.logits.data_ptr(), op.labels.data_ptr(), op.pw_ptr(), op.cw_ptr(), lse_dev.data_ptr(),
            grad_scale, dl.ptr(), ld_d)
    if form == "direct":
        lib.check(L.gs_ce_backward(*head, stream()), "gs_ce_backward")
    elif form == "null":
        lib.check(L.gs_ce_backward_ws(*head, None, 0, stream()), "gs_ce_backward_ws(NULL)")
    else:
        assert form == "ws"
        ws = Workspace(L.gs_ce_backward_workspace_bytes(op.db(), ld_d))
        lib.check(L.gs_ce_backward_ws(*head, ws.ptr(), ws.need, stream()), "gs_ce_backward_ws")
        ws.check()
    got = dl.get("dlogits " + form).view(n, h, w, ld_d)
    assert not bool(got[..., cls:].any()), "dlogits %s: the pad columns Cls..ld_d-1 must be exactly 0.0" % form
    return got[..., :cls].contiguous()


def backward_variants(case):
    """(weighted, layout, ld_d, grad_scale index) -- every combination"""
    cls = case.shape[1]
    return [(wt, lay, ld, gi) for wt in (False, True) for lay in LAYOUTS for ld in (cls, round_up(cls, 4) + 4)
            for gi in (0, 1)]


def grad_scale_of(case, gi):
    n = case.shape[0]
    return (0.4 / (n * case.size[0] * case.size[1]), 1.0)[gi]


def variant_key(case, variant, form):
    return "%s|%s|%s|%d|%d|%s" % ((case.name,) + tuple(variant) + (form,))


# ---- the GS_CE_ROWCLS child -----------------------------------------------------------------------------------
def main(argv):
    """``python tests/util_ce.py DEFAULTS.pt``: the row-tile cases through gs_ce_backward_ws with a workspace,
    in a process whose environment selects another ce_bwd_rowtile_kernel instantiation (GS_CE_ROWCLS is read
    once per process).  Same float64 bound, guards and sentinels as the parent's test; DEFAULTS.pt holds the
    parent's results of the default instantiation, against which bit-identity is reported (not asserted: the
    compiler may contract each instantiation differently)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from conftest import rel_err
    from gaia_seg_amd.hip import lib
    L = lib.load()
    defaults = torch.load(argv[1])
    print("GS_CE_ROWCLS=%s" % os.environ.get("GS_CE_ROWCLS"))
    for case in ROWTILE_CASES:
        worst, same = 0.0, True
        for variant in backward_variants(case):
            weighted, layout, ld_d, gi = variant
            op = Operands(case, layout, weighted)
            ref = ce_ref(case.name, weighted)
            gs = grad_scale_of(case, gi)
            _, lse = run_forward(L, op)
            lse_dev = lse.to(DEV)
            got = run_backward(L, op, lse_dev, "ws", ld_d, gs)
            again = run_backward(L, op, lse_dev, "ws", ld_d, gs)
            assert torch.equal(got, again), "%s: two runs differ" % case.name
            err = rel_err(got, ref.dlogits * gs)
            assert err < TOL, "%s %s: rel_err %.3g" % (case.name, variant, err)
            if case.shape[1] == 1:
                assert not bool(got.any()), "%s: one class, every gradient must be exactly 0.0" % case.name
            worst = max(worst, err)
            same = same and torch.equal(got, defaults[variant_key(case, variant, "ws")])
        print("%-20s dlogits %.2e  bit-identical to the default instantiation: %s" % (case.name, worst, same))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
