"""Helpers of the channel-wise distillation tests: the fp64 restatement of the loss (the witness: the
reference project has no such loss), a pure-Python restatement of the one-pass partial state and its
combine (the algebra csrc/cwd.hip relies on), the operator case table and its seeded inputs."""
import functools
import math

import torch

# The three lines of the definition (mmrazor's ChannelWiseDivergence):
#   phi(x)[n,c,p] = exp(x[n,c,p]/T) / sum_p' exp(x[n,c,p']/T)
#   loss          = weight * T^2 / (N*C) * sum_{n,c} sum_p phi(t) * (log phi(t) - log phi(s))
#   dloss/ds      = weight * T   / (N*C) * (phi(s) - phi(t))


def ref_channel_loss(student, teacher, T, weight):
    n, c = student.shape[:2]
    ls = torch.log_softmax(student.reshape(n * c, -1) / T, dim=1)
    lt = torch.log_softmax(teacher.reshape(n * c, -1) / T, dim=1)
    return weight * T * T / (n * c) * torch.sum(lt.exp() * (lt - ls))


def ref_channel_grad(student, teacher, T, weight):
    n, c = student.shape[:2]
    ps = torch.softmax(student.reshape(n * c, -1) / T, dim=1)
    pt = torch.softmax(teacher.reshape(n * c, -1) / T, dim=1)
    return (weight * T / (n * c) * (ps - pt)).reshape(student.shape)


# ---- the one-pass state of one column (n, c) and its combine, in Python floats (fp64) ----
def segment_state(s, t, T):
    """(m_s, Z_s, m_t, Z_t, A) of a non-empty run of pixels."""
    ms, mt = max(s), max(t)
    zs = sum(math.exp((x - ms) / T) for x in s)
    et = [math.exp((x - mt) / T) for x in t]
    return ms, zs, mt, sum(et), sum(e * (tt - ss) / T for e, tt, ss in zip(et, t, s))


def combine_states(a, b, T):
    ms, mt = max(a[0], b[0]), max(a[2], b[2])
    ras, rbs = math.exp((a[0] - ms) / T), math.exp((b[0] - ms) / T)
    rat, rbt = math.exp((a[2] - mt) / T), math.exp((b[2] - mt) / T)
    return ms, a[1] * ras + b[1] * rbs, mt, a[3] * rat + b[3] * rbt, a[4] * rat + b[4] * rbt


def state_kl(st, T):
    ms, zs, mt, zt, a = st
    return a / zt + (ms - mt) / T + math.log(zs) - math.log(zt)


def state_lse(st, T):
    return st[0] / T + math.log(st[1]), st[2] / T + math.log(st[3])


# ---- operator cases ------------------------------------------------------------------------------
# The forward kernel's split (csrc/cwd.hip cwd_plan): a workgroup of 256 threads holds qb channel units
# side by side (a unit: a channel quad on the float4 path, one channel on the scalar path) and 256 / qb
# pixel slots, and a split leaves every thread at least 8 pixels.  C = 19 channels-last: 5 quads,
# qb = 8, 32 slots: ONE workgroup spans up to 256 pixels of a class map.
SPAN_C19_NHWC = 256

# tag: (N, C, H, W, layout, T, weight, kind)
#   layout "nhwc": padded channels-last views, pixel stride round_up(C, 4) for the student (20 at C = 19)
#                  and 4 more for the teacher (24), pad columns 3.25;  "nchw": plain contiguous tensors
#   kind   "randn" | "large" (uniform in [-80, 80]) | "special" (ramp and constant columns) |
#          "same" (the teacher holds the student's values in the student's layout)
CASES = {
    "c19_p63": (2, 19, 7, 9, "nhwc", 1.0, 1.0, "randn"),          # less than one wave per quad
    "c19_p258": (2, 19, 3, 86, "nhwc", 0.5, 5.0, "randn"),        # just above one workgroup's span
    "c19_p517": (2, 19, 11, 47, "nhwc", 4.0, 1.0, "randn"),       # three ranges, the last one ragged
    "c3": (2, 3, 5, 7, "nhwc", 1.0, 1.0, "randn"),                # a partial quad only
    "c4": (2, 4, 8, 8, "nhwc", 0.5, 1.0, "randn"),                # one full quad
    "c150": (2, 150, 16, 24, "nhwc", 1.0, 5.0, "randn"),          # many quads (five groups), split
    "nchw_c19": (2, 19, 11, 47, "nchw", 1.0, 1.0, "randn"),       # the scalar path, split
    "nchw_c3": (2, 3, 5, 7, "nchw", 4.0, 1.0, "randn"),
    "large": (2, 19, 11, 47, "nhwc", 0.5, 1.0, "large"),          # overflows without the max subtraction
    "special": (2, 19, 11, 47, "nhwc", 1.0, 1.0, "special"),
    "special_nchw": (2, 5, 11, 47, "nchw", 0.5, 1.0, "special"),
}
ZERO_CASES = {
    "p1": (2, 19, 1, 1, "nhwc", 1.0, 1.0, "randn"),               # a 1 x 1 map: loss and gradient 0
    "p1_nchw": (2, 19, 1, 1, "nchw", 0.5, 1.0, "randn"),
    "same": (2, 19, 11, 47, "nhwc", 1.0, 1.0, "same"),
    "same_nchw": (2, 19, 11, 47, "nchw", 4.0, 1.0, "same"),
}


def round_up(x, m):
    return (x + m - 1) // m * m


def _seed(tag):
    return 1000 + sorted(list(CASES) + list(ZERO_CASES)).index(tag)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(student, teacher) as fp32 CPU tensors [N, C, H, W] (contiguous; the layout is applied on upload)."""
    n, c, h, w, _layout, _T, _wgt, kind = (CASES.get(tag) or ZERO_CASES[tag])
    g = torch.Generator().manual_seed(_seed(tag))
    if kind == "large":
        s = (torch.rand(n, c, h, w, generator=g) * 2 - 1) * 80
        t = (torch.rand(n, c, h, w, generator=g) * 2 - 1) * 80
    else:
        s = torch.randn(n, c, h, w, generator=g) * 2
        t = s * 0.5 + torch.randn(n, c, h, w, generator=g) * 1.5
    if kind == "special":
        ramp = (torch.arange(h * w, dtype=torch.float32) * 0.03125).reshape(h, w)
        s[:, 0] = ramp            # the running maximum changes at every pixel ...
        s[:, 1] = -ramp           # ... and never after the first
        s[:, 2] = 1.75            # a constant column
        t[:, 3] = ramp
        t[:, 4] = -0.5
        t[1, 0] = -ramp
    if kind == "same":
        t = s.clone()
    return s, t


@functools.lru_cache(maxsize=None)
def reference(tag):
    """fp64 loss and gradient, and the errors of torch's fp32 CPU evaluation of the same formula against
    them: (loss64, grad64, fp32 loss relative error, fp32 gradient error / largest |grad64|)."""
    _n, _c, _h, _w, _layout, T, wgt, _kind = (CASES.get(tag) or ZERO_CASES[tag])
    s, t = inputs(tag)
    l64 = ref_channel_loss(s.double(), t.double(), T, wgt)
    g64 = ref_channel_grad(s.double(), t.double(), T, wgt)
    l32 = ref_channel_loss(s, t, T, wgt)
    g32 = ref_channel_grad(s, t, T, wgt)
    gmax = float(g64.abs().max())
    e_l = abs(float(l32) - float(l64)) / abs(float(l64)) if float(l64) != 0 else 0.0
    e_g = float((g32.double() - g64).abs().max()) / gmax if gmax != 0 else 0.0
    return float(l64), g64, e_l, e_g


def padded(x, ld, device):
    """[n, c, h, w] values of ``x`` as a view of a padded NHWC buffer whose pad columns hold 3.25."""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), 3.25)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.to(device).permute(0, 3, 1, 2)[:, :c]


def upload(tag, device="cuda"):
    """The case's two maps on the device in the case's layout."""
    _n, c, _h, _w, layout, _T, _wgt, kind = (CASES.get(tag) or ZERO_CASES[tag])
    s, t = inputs(tag)
    if layout == "nchw":
        return s.to(device).contiguous(), t.to(device).contiguous()
    ld = round_up(c, 4)
    return padded(s, ld, device), padded(t, ld if kind == "same" else ld + 4, device)
