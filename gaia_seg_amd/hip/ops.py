"""Tape-aware operators: each function launches the forward HIP kernel(s) through the C-ABI and
records the closure that launches the backward kernel(s).

Nothing in this file computes with torch ops on the data path; torch is used for allocation
and (SyncBN only) the tiny statistics exchange over RCCL.

This module is the operator catalogue and the home of the policy flags (SIDE_WGRAD, BRANCH_*,
DEFER_*: whether an op uses the side stream, a branch stream or a deferred BatchNorm).  The streams
themselves, their scratch and the scopes that switch them are ``streams``; ``Act`` and the tape are
``runtime``.  Imports go one way: lib <- streams <- runtime <- ops.

Every backward closure gets the buffers its kernel writes from shared helpers: ``_input_grad`` /
``_grad_target`` (the gradient of an input activation, and the ONE rule for the accumulate flag),
``_sole_grad`` (of an input whose kernel has no accumulate form) and ``_param_grad`` (of a parameter,
followed by ``_notify_params`` after the launch).  ``_qkv_attention`` is the body of the q / k / v ops.
"""
import ctypes
import os

import torch

from . import lib as _lib
from . import streams as _streams
from .runtime import Act, round_up
from .streams import WORKSPACE as _ws
from .streams import _notify, current_stream_ptr

# Policy: which ops use the streams of ``streams``.  GS_SIDE_WGRAD=0 keeps the conv weight gradients
# on the stream of their data gradients; GS_BRANCH_SHORTCUT / GS_BRANCH_AUX switch the two uses of the
# branch streams separately (GS_BRANCH=0, read by ``streams``, switches both off).
SIDE_WGRAD = os.environ.get("GS_SIDE_WGRAD", "1") != "0"
BRANCH_SHORTCUT = _streams.BRANCH and os.environ.get("GS_BRANCH_SHORTCUT", "1") != "0"
BRANCH_AUX = _streams.BRANCH and os.environ.get("GS_BRANCH_AUX", "1") != "0"
BRANCH_SHORTCUT_MAX_GFLOP = float(os.environ.get("GS_BRANCH_SHORTCUT_MAX_GFLOP", "8"))


def _L():
    return _lib.load()


_INT32_ARRAYS = {}


def _int32_array(n):
    """ctypes array type of n int32 (cached: creating the type per call leaves a cycle of type
    objects for the garbage collector at every step)."""
    t = _INT32_ARRAYS.get(n)
    if t is None:
        t = _INT32_ARRAYS[n] = ctypes.c_int32 * n
    return t


def ensure_grad(param):
    """``param.grad`` with the physical layout of ``param`` (zeros on first use).

    Parameters with a padded / permuted physical layout (HWIO conv weights, the padded conv_seg
    bias) carry a ``_gs_grad_factory`` that allocates matching storage; with a ParamArena installed
    the gradients already exist as views of the flat gradient buffer."""
    g = param.grad
    if g is not None and g.stride() == param.stride():   # the common case, checked first
        return g
    if param.grad is None:
        factory = getattr(param, "_gs_grad_factory", None)
        if factory is not None:
            param.grad = factory()
        else:
            param.grad = torch.zeros_like(param, memory_format=torch.preserve_format)
    if param.grad.stride() != param.stride():
        raise RuntimeError("gradient layout %s differs from parameter layout %s"
                           % (param.grad.stride(), param.stride()))
    return param.grad


conv_out_size = _lib.conv_out_size


def _conv_desc(x, weight, co, stride, pad, dil, ldy, ld_add=0, role=0):
    """gs_conv_desc for activation ``x`` and a max-size weight Parameter (logical OIHW, physical
    HWIO with row pitch ``Co_ld``): lib.conv_desc with the strides of ``x`` (the stem's NCHW image
    is not packed NHWC)."""
    co_max, ci_max, kh, kw = weight.shape
    if x.nchw_image:
        n, c, h, w = x.t.shape
    else:
        n, h, w, c = x.t.shape
    d = _lib.conv_desc(n, h, w, c, co, (kh, kw), stride, dil, pad, ci_max, weight.stride(1), ldy=ldy,
                       ld_add=ld_add, role=role)
    if x.nchw_image:
        d.x_sn, d.x_sc, d.x_sh, d.x_sw = x.t.stride()
    else:
        d.x_sn, d.x_sh, d.x_sw, d.x_sc = x.t.stride()
    if c > ci_max:
        raise ValueError("input has %d channels, conv supports at most %d" % (c, ci_max))
    return d


class KernelTimer:
    """Optional HIP-event timing of tagged kernel launches on the current stream (bench.py uses it
    to time the dynamic 3x3 bottleneck conv inside real training steps)."""

    def __init__(self):
        self.records = {}   # tag -> list of (start_event, end_event, flops)

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, tag, start, flops):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.setdefault(tag, []).append((start, e, flops))

    def summary(self):
        """tag -> (launches, total_ms, total_flops); call after a device synchronize."""
        out = {}
        for tag, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            out[tag] = (len(recs), ms, float(sum(f for _, _, f in recs)))
        return out


TIMER = None  # set to a KernelTimer to enable

# Diagnostics: when set to a list, every BatchNorm(+residual)+ReLU records (gamma Parameter,
# bool NHWC tensor "output > 0", taken at once: UPer's top-down add later updates outputs in place).  The gradient-parity tests use it to evaluate the CPU
# oracle on the same ReLU branch pattern as this path (tests/conftest.py).  None = off (no cost).
RELU_TRACE = None
POOL_TRACE = None   # same, for MaxPool2d: list of uint8 [N, Ho, Wo, C] argmax tap tensors (kh * k + kw)


def _trace_relu(bn, out):
    if RELU_TRACE is not None and bn.weight is not None:
        RELU_TRACE.append((bn.weight, out.t > 0))


def _trace_relu_deferred(bn, y, coeffs):
    """Same for a deferred BN+ReLU: the mask comes from the real apply kernel (same expression as the
    fused loaders and the backward mask), run into a scratch buffer only while tracing."""
    if RELU_TRACE is not None and bn.weight is not None:
        tmp = Act.empty(y.N, y.H, y.W, y.C, y.t.device)
        _lib.check(_L().gs_bn_apply(y.ptr, y.rows, y.C, y.ld, coeffs.data_ptr(), None, 0, 1, tmp.ptr,
                                    tmp.ld, current_stream_ptr()), "gs_bn_apply")
        RELU_TRACE.append((bn.weight, tmp.t > 0))


# Loader fusion of BN + ReLU into the consumer convolution (gs_conv_desc.in_affine).  Which edges of
# a bottleneck use it: "conv3" = bn2 -> conv3 (1x1), "conv2" = bn1 -> conv2 (the 3x3, K3).
# GS_DEFER_BN = comma list, "all" or "none".  r02 A/B on the sampled mix (bench.py, 30 steps):
# none 145.5 img/s, K3 at 0.555 of peak; all 145.4 img/s, K3 at 0.500 (the affine + select in the
# store slot of the K loop costs the 3x3 what the two removed bn_apply launches save); the default
# keeps the headline 3x3 kernel free of it.
_defer = os.environ.get("GS_DEFER_BN", "conv3").lower()
DEFER_EDGES = {"all": {"conv2", "conv3"}, "none": set()}.get(_defer, set(_defer.split(",")))
DEFER_BN = True   # master switch (tests flip it to compare the two forms bit for bit)
# the projection shortcut's BatchNorm inside the block's last apply pass (gs_bn_args.residual_coeffs)
DEFER_SHORTCUT_BN = os.environ.get("GS_DEFER_SHORTCUT_BN", "1") != "0"


def _materialize(tape, x, coeffs, relu):
    z = Act.empty(x.N, x.H, x.W, x.C, x.t.device)
    _lib.check(_L().gs_bn_apply(x.ptr, x.rows, x.C, x.ld, coeffs.data_ptr(), None, 0, relu, z.ptr, z.ld,
                                current_stream_ptr()), "gs_bn_apply")
    z.requires_grad = x.requires_grad
    add_grad_passthrough(tape, x, z)
    return z


def materialize(tape, x):
    """Write out relu(bn(t)) of a deferred activation (consumers without the loader fusion)."""
    return x if x.affine is None else _materialize(tape, x, x.affine, 1)


def materialize_residual(tape, r):
    """Write out bn(t) of a residual whose BatchNorm was left to its consumer (Act.res_affine), for
    consumers that take a plain addend."""
    return r if r is None or r.res_affine is None else _materialize(tape, r, r.res_affine, 0)


# ---- forward precision (inference) -----------------------------------------------------------
# gs_set_forward_precision: 0 = fp32 (default), 1 = the fast forward launches contract fp16-rounded
# operands with fp32 accumulation (include/gaiaseg_hip.h).  The library picks the K loop and the
# tile at launch time from the switch: neither the workspace size nor anything in the conv_bn plan
# cache (_ConvBnPlan) depends on it, so the cache keys do not carry it.  This mirror of the switch
# lets conv2d / conv_bn refuse a recording tape without a library call per layer.
_PRECISIONS = {"fp32": _lib.PRECISION_FP32, "fp16": _lib.PRECISION_FP16}
FORWARD_PRECISION = _lib.PRECISION_FP32


def _check_mode(what, mode):
    if mode not in _PRECISIONS:
        raise ValueError("%s precision must be one of %s, got %r" % (what, sorted(_PRECISIONS), mode))


def _set_precision(what, mode, current):
    """Set the library's ``what`` ('forward' / 'train') precision to 'fp32' / 'fp16'; returns the
    previous name (``current()``: the library's mode before the call)."""
    _check_mode(what, mode)
    prev = "fp16" if current() == _lib.PRECISION_FP16 else "fp32"
    name = "gs_set_%s_precision" % what
    _lib.check(getattr(_L(), name)(_PRECISIONS[mode]), name)
    return prev


def set_forward_precision(mode):
    """Set the library's forward precision ('fp32' / 'fp16'); returns the previous name."""
    global FORWARD_PRECISION
    prev = _set_precision("forward", mode, lambda: FORWARD_PRECISION)
    FORWARD_PRECISION = _PRECISIONS[mode]
    return prev


# ---- training precision ----------------------------------------------------------------------
# gs_set_train_precision: 1 = the forward launches of the fp16 inference mode AND the fast
# data-gradient launches contract fp16-rounded operands (weight gradients, BN, loss and SGD stay
# fp32).  Separate from the inference switch: FORWARD_PRECISION and
# gs_get_forward_precision() keep reading fp32 while training runs in fp16.  As for the forward
# switch, neither workspace sizes nor the conv_bn plan cache depend on it.
def set_train_precision(mode):
    """Set the library's training precision ('fp32' / 'fp16'); returns the previous name."""
    return _set_precision("train", mode, lambda: _L().gs_get_train_precision())


class _precision_scope:
    """``with <scope>(mode): ...`` -- the previous precision is restored on exit, exceptions included."""
    what = set = None

    def __init__(self, mode):
        _check_mode(self.what, mode)
        self.mode = mode
        self._prev = None

    def __enter__(self):
        self._prev = self.set(self.mode)
        return self

    def __exit__(self, *exc):
        self.set(self._prev)
        return False


class forward_precision(_precision_scope):
    """``with forward_precision("fp16"): ...`` -- inference forwards with fp16 operands.  A conv that
    records a tape (training) inside raises: the backward kernels assume an fp32 forward."""
    what, set = "forward", staticmethod(set_forward_precision)


class train_precision(_precision_scope):
    """``with train_precision("fp16"): ...`` -- training steps with fp16 conv operands (forward and
    data gradient)."""
    what, set = "train", staticmethod(set_train_precision)


def _check_precision(tape):
    if FORWARD_PRECISION != _lib.PRECISION_FP32 and tape.enabled:
        raise RuntimeError("fp16 forward precision is inference only: a conv was called with a "
                           "recording tape (training) inside forward_precision('fp16')")


def conv2d(tape, x, weight, bias, co, stride=1, pad=0, dil=1, out=None, tag=None):
    """DynConv2d forward: y = conv(x, weight[:co, :x.C]) (+ bias[:co]).

    ``co`` is the active output width; the active input width is x.C."""
    _check_precision(tape)
    L = _L()
    x = materialize(tape, x)
    co_eff = round_up(co, 4)
    dev = x.t.device
    kh, kw = weight.shape[2], weight.shape[3]
    if x.nchw_image:
        n, _, h, w = x.t.shape
    else:
        n, h, w, _ = x.t.shape
    ho, wo = conv_out_size(h, kh, stride, pad, dil), conv_out_size(w, kw, stride, pad, dil)
    if out is None:
        out = Act.empty(n, ho, wo, co, dev)
    d = _conv_desc(x, weight, co_eff, stride, pad, dil, out.ld, role=1 if tag == "k3" else 0)
    need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
    ws = _ws.get(need, dev)
    st = current_stream_ptr()
    timed = TIMER is not None and tag is not None
    if timed:
        t0 = TIMER.begin()
    _lib.check(L.gs_conv2d_forward(ctypes.byref(d), x.ptr, weight.data_ptr(),
                                   bias.data_ptr() if bias is not None else None, None, out.ptr,
                                   ws.data_ptr(), ws.numel(), st), "gs_conv2d_forward")
    if timed:
        ci = x.t.shape[1] if x.nchw_image else x.C
        TIMER.end(tag + ".fwd", t0, 2.0 * n * ho * wo * co * ci * kh * kw)

    def backward():
        dy = out.g
        if dy is None:
            return
        ws_b = _ws.get(need, dev)
        s = current_stream_ptr()
        if weight.requires_grad:
            gw = ensure_grad(weight)
            if SIDE_WGRAD:
                _streams.queue_wgrad(d, x, dy, weight, gw, need, dev)   # notifies when launched
            else:
                _lib.check(L.gs_conv2d_wgrad(ctypes.byref(d), x.ptr, dy.data_ptr(), gw.data_ptr(),
                                             ws_b.data_ptr(), ws_b.numel(), s), "gs_conv2d_wgrad")
                _notify(weight)
        if bias is not None and bias.requires_grad:
            gb = ensure_grad(bias)
            rows = out.rows
            nb = L.gs_colsum_workspace_bytes(rows, co_eff)
            wsb = _ws.get(nb, dev)
            # the padded bias storage holds co_eff floats; the sum of the pad column is zero
            _lib.check(L.gs_colsum(dy.data_ptr(), rows, co_eff, out.ld, gb.data_ptr(),
                                   wsb.data_ptr(), wsb.numel(), s), "gs_colsum")
            _notify(bias)
        if x.requires_grad:
            acc = _input_grad(x)
            _lib.check(L.gs_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), weight.data_ptr(),
                                         x.g.data_ptr(), acc, ws_b.data_ptr(),
                                         ws_b.numel(), s), "gs_conv2d_dgrad")

    tape.record(backward)
    return out


def dwconv2d(tape, x, weight, pad, dil=1, out=None, bias=None):
    """Depthwise 3x3 or 7x7 DynConv2d forward (stride 1): y = conv(x, weight[:x.C], groups = x.C)
    (+ bias[:x.C]).

    ``weight`` is the max-size Parameter, logical [C_max, 1, K, K], physical HWIO [K][K][1][C_ld]; the
    active width is x.C.  fp32 in every precision mode (the kernels are bandwidth-bound); everything
    runs on the current stream, the weight gradient included."""
    _check_precision(tape)
    L = _L()
    x = materialize(tape, x)
    c_max, ci, kh, kw = weight.shape
    c = x.C
    if ci != 1 or (kh, kw) not in ((3, 3), (7, 7)):
        raise ValueError("dwconv2d needs a [C, 1, 3, 3] or [C, 1, 7, 7] weight, got %s"
                         % (tuple(weight.shape),))
    if c > c_max:
        raise ValueError("input has %d channels, conv supports at most %d" % (c, c_max))
    if c % 4:
        raise ValueError("dwconv2d needs a channel count that is a multiple of 4, got %d" % c)
    dev = x.t.device
    ho, wo = conv_out_size(x.H, kh, 1, pad, dil), conv_out_size(x.W, kw, 1, pad, dil)
    if out is None:
        out = Act.empty(x.N, ho, wo, c, dev)
    d = _lib.dwconv_desc(x.N, x.H, x.W, c, pad, dil, c_ld=weight.stride(1), ldx=x.ld, ldy=out.ld, k=kh)
    _lib.check(L.gs_dwconv2d_forward(ctypes.byref(d), x.ptr, weight.data_ptr(),
                                     bias.data_ptr() if bias is not None else None, out.ptr,
                                     current_stream_ptr()), "gs_dwconv2d_forward")

    def backward():
        dy = out.g
        if dy is None:
            return
        s = current_stream_ptr()
        db = ctypes.byref(d)
        if weight.requires_grad:
            gw = ensure_grad(weight)
            need = L.gs_dwconv2d_workspace_bytes(db)
            ws = _ws.get(need, dev)
            _lib.check(L.gs_dwconv2d_wgrad(db, x.ptr, dy.data_ptr(), gw.data_ptr(), ws.data_ptr(),
                                           ws.numel(), s), "gs_dwconv2d_wgrad")
            _notify(weight)
        if bias is not None and bias.requires_grad:
            gb = ensure_grad(bias)
            nb = L.gs_colsum_workspace_bytes(out.rows, c)
            wsb = _ws.get(nb, dev)
            _lib.check(L.gs_colsum(dy.data_ptr(), out.rows, c, out.ld, gb.data_ptr(), wsb.data_ptr(),
                                   wsb.numel(), s), "gs_colsum")
            _notify(bias)
        if x.requires_grad:
            acc = _input_grad(x)
            _lib.check(L.gs_dwconv2d_dgrad(db, dy.data_ptr(), weight.data_ptr(), x.g.data_ptr(), acc,
                                           s), "gs_dwconv2d_dgrad")

    tape.record(backward)
    return out


def _active_width(x, param, what):
    c = x.C
    if c > param.shape[-1]:     # the channels are the last dimension of a parameter ([C] or [1, 1, 1, C])
        raise ValueError("input has %d channels, %s supports at most %d" % (c, what, param.shape[-1]))
    if c % 4:
        raise ValueError("%s needs a channel count that is a multiple of 4, got %d" % (what, c))
    return c


def _input_grad(x):
    """Make sure ``x.g`` exists and return the accumulate flag of the kernel that writes it.

    THE RULE, for every tape op: the flag is "the target held something before this call" -- 1 when
    x.g already existed, else 0 after allocating it.  No op overrides it.  It is right for a channel
    slice too: the gradient of the buffer that owns the slice is allocated zeroed, and the slices of an
    activation are disjoint column ranges, so no kernel has written this slice's columns yet and a
    plain write (which does not read the old gradient) leaves the siblings' zeros alone.  A slice whose
    sibling already allocated the owner's gradient reports 1 and accumulates onto those zeros."""
    if x.g is not None:
        return 1
    root = x
    while root.parent is not None:
        root = root.parent
    if root is x:
        x.new_grad()
    elif root.g is None:
        root.new_grad().zero_()
    return 0


def _sole_grad(x, sole):
    """``x.g``, fresh, for a kernel with no accumulate form: this op must be the only consumer of the
    input that ``sole`` names, so a gradient that is already held raises (before anything is
    allocated).  Not exact for slices, on the safe side: a sibling slice that allocated the owner's
    gradient makes it raise as well."""
    if _input_grad(x):
        raise RuntimeError("%s has more than one consumer; unsupported" % sole)
    return x.g


def _grad_target(x, sole=None):
    """Where a kernel that always produces the gradient of its input ``x`` writes it -> (tensor,
    accumulate flag).  An input that requires a gradient gets ``x.g`` with the flag of
    ``_input_grad``, or with ``sole`` given the fresh one of ``_sole_grad``.  An input that needs none
    gets scratch with x's own shape AND pitch (flag 0): a kernel that addresses the gradient with the
    descriptor's ``ldx`` may rely on that, every other caller passes the ``stride(2)`` of what it got."""
    if not x.requires_grad:
        return Act.empty(x.N, x.H, x.W, x.C, x.t.device, ld=x.ld).t, 0
    if sole:
        return _sole_grad(x, sole), 0
    acc = _input_grad(x)
    return x.g, acc


def _param_grad(param):
    """Where a kernel that always produces the gradient of ``param`` writes it: param.grad, or scratch
    with the parameter's layout for a frozen one (the kernels address it with the parameter's pitch).
    ``_notify_params`` follows the launch."""
    return ensure_grad(param) if param.requires_grad else torch.empty_like(param)


def _notify_params(*params):
    """After the launch that wrote them: the gradients of those ``params`` that take one are ready."""
    for p in params:
        if p is not None and p.requires_grad:
            _notify(p)


def layernorm(tape, x, weight, bias, eps=1e-6, out=None):
    """DynLN forward: LayerNorm over the x.C active channels of every pixel with weight[:x.C], bias[:x.C]
    (the reference's channels_first and channels_last forms are this one kernel on NHWC storage).
    The per-pixel mean and 1/std are kept for the backward."""
    L = _L()
    x = materialize(tape, x)
    c = _active_width(x, weight, "layernorm")
    dev, rows = x.t.device, x.rows
    if out is None:
        out = Act.empty(x.N, x.H, x.W, c, dev)
    stats = torch.empty(2 * rows, dtype=torch.float32, device=dev)
    mean_ptr, rstd_ptr = stats.data_ptr(), stats.data_ptr() + 4 * rows
    d = _lib.layernorm_desc(rows, c, eps, ldx=x.ld, ldy=out.ld)
    _lib.check(L.gs_layernorm_forward(ctypes.byref(d), x.ptr, weight.data_ptr(), bias.data_ptr(), out.ptr,
                                      mean_ptr, rstd_ptr, current_stream_ptr()), "gs_layernorm_forward")

    def backward():
        dy = out.g
        if dy is None:
            return
        keep = stats  # noqa: F841 -- the closure owns the storage behind mean_ptr / rstd_ptr
        db = ctypes.byref(d)
        gw, gb = _param_grad(weight), _param_grad(bias)
        ws = _ws.get(L.gs_layernorm_workspace_bytes(db), dev)
        dx, acc = _grad_target(x)   # (addressed with d.ldx)
        _lib.check(L.gs_layernorm_backward(db, x.ptr, dy.data_ptr(), weight.data_ptr(), mean_ptr, rstd_ptr,
                                           dx.data_ptr(), gw.data_ptr(), gb.data_ptr(), acc, ws.data_ptr(),
                                           ws.numel(), current_stream_ptr()), "gs_layernorm_backward")
        _notify_params(weight, bias)

    tape.record(backward)
    return out


def gelu(tape, x, out=None):
    """nn.GELU() (exact erf form).  The backward recomputes the derivative from x."""
    L = _L()
    x = materialize(tape, x)
    if x.C % 4:
        raise ValueError("gelu needs a channel count that is a multiple of 4, got %d" % x.C)
    if out is None:
        out = Act.empty(x.N, x.H, x.W, x.C, x.t.device)
    _lib.check(L.gs_gelu_forward(x.ptr, out.ptr, x.rows, x.C, x.ld, out.ld, current_stream_ptr()),
               "gs_gelu_forward")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        dx = _sole_grad(x, "GELU input")
        _lib.check(L.gs_gelu_backward(x.ptr, dy.data_ptr(), dx.data_ptr(), x.rows, x.C, x.ld, dy.stride(2),
                                      dx.stride(2), current_stream_ptr()), "gs_gelu_backward")

    tape.record(backward)
    return out


def gelu_grn(tape, x, weight, bias, eps=1e-6, out=None):
    """ConvNeXt V2's hidden activation in one operator: Global Response Normalization of a = GELU(x) over
    the x.C active channels, y = a * (1 + weight[:C] * Nx) + bias[:C] with Nx = G / (mean_c G + eps) and
    G[n, c] the 2-norm of a over the pixels of sample n.  ``weight`` / ``bias`` are the max-size vectors
    (any shape whose last dimension holds the channels, transformers' [1, 1, 1, C]).  a is never stored:
    G [N, C] is kept, and the backward recomputes a from x."""
    L = _L()
    x = materialize(tape, x)
    c = _active_width(x, weight, "gelu_grn")
    if weight.numel() != weight.shape[-1] or bias.shape != weight.shape:
        raise ValueError("gelu_grn: weight %s / bias %s are not per-channel vectors" % (tuple(weight.shape),
                                                                                      tuple(bias.shape)))
    dev = x.t.device
    if out is None:
        out = Act.empty(x.N, x.H, x.W, c, dev)
    G = torch.empty(x.N * c, dtype=torch.float32, device=dev)
    d = _lib.gelu_grn_desc(x.N, x.H * x.W, c, eps, ldx=x.ld, ldy=out.ld, lddy=out.ld, lddx=x.ld)
    ws = _ws.get(L.gs_gelu_grn_workspace_bytes(ctypes.byref(d)), dev)
    _lib.check(L.gs_gelu_grn_forward(ctypes.byref(d), x.ptr, weight.data_ptr(), bias.data_ptr(), out.ptr,
                                     G.data_ptr(), ws.data_ptr(), ws.numel(), current_stream_ptr()),
               "gs_gelu_grn_forward")

    def backward():
        dy = out.g
        if dy is None:
            return
        gw, gb = _param_grad(weight), _param_grad(bias)
        dx, _ = _grad_target(x, "gelu_grn input")
        d.lddy, d.lddx = dy.stride(2), dx.stride(2)
        db = ctypes.byref(d)
        ws = _ws.get(L.gs_gelu_grn_workspace_bytes(db), dev)
        _lib.check(L.gs_gelu_grn_backward(db, x.ptr, dy.data_ptr(), weight.data_ptr(), G.data_ptr(),
                                          dx.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                          ws.numel(), current_stream_ptr()), "gs_gelu_grn_backward")
        _notify_params(weight, bias)

    tape.record(backward)
    return out


def layer_scale_add(tape, identity, z, gamma, out=None):
    """ConvNeXt's block output: identity + gamma[:C] * z, one kernel.  ``gamma`` None (no layer scale) is
    the plain residual add.  The identity's gradient is the output's, handed on without a copy."""
    L = _L()
    identity, z = materialize(tape, identity), materialize(tape, z)
    c, rows, dev = z.C, z.rows, z.t.device
    if identity.C != c or identity.rows != rows:
        raise ValueError("layer_scale_add: identity %s and branch %s differ" % (tuple(identity.t.shape),
                                                                                  tuple(z.t.shape)))
    if out is None:
        out = Act.empty(z.N, z.H, z.W, c, dev)
    st = current_stream_ptr()
    if gamma is not None:
        _active_width(z, gamma, "layer_scale_add")
        _lib.check(L.gs_layer_scale_add_forward(identity.ptr, z.ptr, gamma.data_ptr(), out.ptr, rows, c,
                                                identity.ld, z.ld, out.ld, st), "gs_layer_scale_add_forward")
    else:
        for src, acc in ((identity, 0), (z, 1)):
            _lib.check(L.gs_copy2d(src.ptr, src.ld, out.ptr, out.ld, rows, c, 1.0, acc, st), "gs_copy2d")

    def backward():
        dout = out.g
        if dout is None:
            return
        s = current_stream_ptr()
        if gamma is None:
            if z.requires_grad:
                # (copied, not aliased: the identity below may alias dout and later add to it)
                acc = _input_grad(z)
                _lib.check(L.gs_copy2d(dout.data_ptr(), dout.stride(2), z.g.data_ptr(), z.g.stride(2), rows, c,
                                       1.0, acc, s), "gs_copy2d")
        else:
            dz = _sole_grad(z, "layer-scaled branch")
            gg = _param_grad(gamma)
            ws = _ws.get(L.gs_layer_scale_workspace_bytes(rows, c), dev)
            _lib.check(L.gs_layer_scale_backward(dout.data_ptr(), z.ptr, gamma.data_ptr(), dz.data_ptr(),
                                                 gg.data_ptr(), rows, c, dout.stride(2), z.ld, dz.stride(2),
                                                 ws.data_ptr(), ws.numel(), s), "gs_layer_scale_backward")
            _notify_params(gamma)
        if identity.requires_grad:
            _pass_residual_grad(L, identity, dout, rows, c, s)

    tape.record(backward)
    return out


def msca(tape, x, unit, out=None):
    """SegNeXt's multi-scale convolutional attention without its 1x1 conv, one operator (gs_msca_*):

        a = conv0(x);  s = a + conv0_2(conv0_1(a)) + conv1_2(conv1_1(a)) + conv2_2(conv2_1(a))

    all depthwise, on the x.C active channels.  ``unit.filters()`` gives the 14 max-size Parameters in the
    order of gs_msca_filters: w0, b0, the three 1xK weights, their biases, the three Kx1 weights, their
    biases (logical [C_max, 1, KH, KW], physical HWIO).  a and the three row results are kept for the
    backward; the input's gradient is added to where it already holds one (x also feeds the gate)."""
    L = _L()
    x = materialize(tape, x)
    params = tuple(unit.filters())
    w0 = params[0]
    c = x.C
    if c > w0.shape[0]:
        raise ValueError("input has %d channels, msca supports at most %d" % (c, w0.shape[0]))
    if c % 4:
        raise ValueError("msca needs a channel count that is a multiple of 4, got %d" % c)
    c_ld = w0.stride(1)
    if any(p.stride(1) != c_ld for p in params[2:5] + params[8:11]):
        raise ValueError("msca: the filters differ in their channel pitch")
    dev = x.t.device
    if out is None:
        out = Act.empty(x.N, x.H, x.W, c, dev)
    d = _lib.msca_desc(x.N, x.H, x.W, c, c_ld=c_ld, ldx=x.ld, lds=out.ld, k0=w0.shape[2],
                       k=tuple(p.shape[3] for p in params[2:5]))
    db = ctypes.byref(d)

    def table(ts):
        ptrs = [t.data_ptr() for t in ts]
        return _lib.msca_filters(ptrs[0], ptrs[1], ptrs[2:5], ptrs[5:8], ptrs[8:11], ptrs[11:14])

    filters = table(params)
    saved = torch.empty(L.gs_msca_saved_bytes(db), dtype=torch.uint8, device=dev)
    _lib.check(L.gs_msca_forward(db, x.ptr, ctypes.byref(filters), out.ptr, saved.data_ptr(),
                                 current_stream_ptr()), "gs_msca_forward")

    def backward():
        ds = out.g
        if ds is None:
            return
        if ds.stride(2) != d.lds:
            raise RuntimeError("msca: the output gradient's pitch %d differs from the output's %d"
                               % (ds.stride(2), d.lds))
        grads = [_param_grad(p) for p in params]
        gtable = table(grads)
        ws = _ws.get(L.gs_msca_workspace_bytes(db), dev)
        dx, acc = _grad_target(x)   # (addressed with d.ldx)
        _lib.check(L.gs_msca_backward(db, x.ptr, ds.data_ptr(), ctypes.byref(filters), saved.data_ptr(),
                                      dx.data_ptr(), acc, ctypes.byref(gtable), ws.data_ptr(), ws.numel(),
                                      current_stream_ptr()), "gs_msca_backward")
        _notify_params(*params)

    tape.record(backward)
    return out


def gate_mul(tape, g, u, out=None):
    """The gate of SegNeXt's attention: y = g * u, elementwise.  The backward writes g's gradient and adds
    u's to where it already holds one (u also feeds the convolutions that produced g)."""
    L = _L()
    g, u = materialize(tape, g), materialize(tape, u)
    c, rows = g.C, g.rows
    if u.C != c or u.rows != rows:
        raise ValueError("gate_mul: %s and %s differ" % (tuple(g.t.shape), tuple(u.t.shape)))
    if c % 4:
        raise ValueError("gate_mul needs a channel count that is a multiple of 4, got %d" % c)
    if out is None:
        out = Act.empty(g.N, g.H, g.W, c, g.t.device)
    _lib.check(L.gs_gate_mul_forward(g.ptr, u.ptr, out.ptr, rows, c, g.ld, u.ld, out.ld,
                                     current_stream_ptr()), "gs_gate_mul_forward")

    def backward():
        dy = out.g
        if dy is None or not (g.requires_grad or u.requires_grad):
            return
        dg, _ = _grad_target(g, "gate_mul's first input")
        du, acc = _grad_target(u)
        _lib.check(L.gs_gate_mul_backward(dy.data_ptr(), g.ptr, u.ptr, dg.data_ptr(), du.data_ptr(), rows, c,
                                          dy.stride(2), g.ld, u.ld, dg.stride(2), du.stride(2), acc,
                                          current_stream_ptr()), "gs_gate_mul_backward")

    tape.record(backward)
    return out


def _attention_f16(f16):
    """Whether an attention op called with ``f16`` takes the fp16-operand entries: only inside an fp16 mode
    (the forward switch, or the library's train precision).  In fp32 modes the flag does nothing."""
    return bool(f16) and (FORWARD_PRECISION == _lib.PRECISION_FP16
                          or _L().gs_get_train_precision() == _lib.PRECISION_FP16)


def _attention_setup(tape, what, q, k, v, heads, scale, out, f16):
    """What ``attention`` and ``attention_relpos`` (``what``) share -> (q, k, v, out, lse, descriptor, suffix
    of the entries to call): q, k and v materialised and checked to be [B, 1, N, 64 * heads], the output and
    the log-sum-exp buffer allocated."""
    sfx = "_f16" if _attention_f16(f16) else ""
    q, k, v = materialize(tape, q), materialize(tape, k), materialize(tape, v)
    c = _lib.ATTENTION_HEAD_DIM * heads
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.C != c or t.rows != q.rows or t.H != 1:
            raise ValueError("%s: %s is %s, expected [B, 1, N, %d] for %d heads"
                             % (what, name, tuple(t.t.shape), c, heads))
    b, n, dev = q.N, q.W, q.t.device
    if out is None:
        out = Act.empty(b, 1, n, c, dev)
    lse = torch.empty(b * heads * n, dtype=torch.float32, device=dev)
    d = _lib.attention_desc(b, n, heads, scale, ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    return q, k, v, out, lse, d, sfx


def _qkv_attention(tape, stem, sfx, d, q, k, v, out, lse, table=None):
    """The body ``attention``, ``attention_kv`` and ``window_attention`` share once the op has checked its
    shapes and filled its descriptor ``d``: the call of <stem>_forward<sfx> and the recorded backward
    (<stem>_backward<sfx> with a pooled workspace of <stem>_workspace_bytes<sfx>).  The backward kernels take
    ONE accumulate flag for the three gradients: some gradient of q, k, v was held before this call (the
    rule of ``_input_grad``); with it set, those that start fresh are zeroed.  q, k and v are distinct
    activations or disjoint slices.  ``table``: window_attention's bias table, passed after v; its
    gradient goes after dv, its active columns start from zero under the flag, and it is notified."""
    L = _L()
    fwd, bwd, ws_bytes = (getattr(L, "%s_%s%s" % (stem, e, sfx)) for e in ("forward", "backward", "workspace_bytes"))
    dev = q.t.device
    inputs = (q, k, v) if table is None else (q, k, v, table)
    _lib.check(fwd(ctypes.byref(d), q.ptr, k.ptr, v.ptr, *(t.data_ptr() for t in inputs[3:]), out.ptr,
                   lse.data_ptr(), current_stream_ptr()), "%s_forward%s" % (stem, sfx))

    def backward():
        dy = out.g
        if dy is None or not any(t.requires_grad for t in inputs):
            return
        acc = 1 if any(t.g is not None for t in (q, k, v)) else 0
        for t in (q, k, v):
            if not _input_grad(t) and acc:
                t.g.zero_()
        d.lddq, d.lddk, d.lddv, d.lddo = q.g.stride(2), k.g.stride(2), v.g.stride(2), dy.stride(2)
        grads = [q.g, k.g, v.g]
        if table is not None:
            grads.append(_param_grad(table))
            if acc:   # the flag covers the table too: its active columns start from zero
                grads[3][:, :d.heads].zero_()
        db = ctypes.byref(d)
        ws = _ws.get(ws_bytes(db), dev)
        _lib.check(bwd(db, q.ptr, k.ptr, v.ptr, *(t.data_ptr() for t in inputs[3:]), out.ptr, lse.data_ptr(),
                       dy.data_ptr(), *(g.data_ptr() for g in grads), acc, ws.data_ptr(), ws.numel(),
                       current_stream_ptr()), "%s_backward%s" % (stem, sfx))
        _notify_params(table)

    tape.record(backward)
    return out


def attention(tape, q, k, v, heads, scale, out=None, f16=False):
    """Multi-head softmax self-attention, head dimension 64: ``heads`` active heads in the leading
    64 * heads columns of q, k and v (token activations [B, 1, N, 64 * heads], each with its own pitch: three
    column slices of one buffer are fine).  No N x N matrix is stored; the log-sum-exp of every query row is
    kept for the backward, which recomputes the probabilities.  ``f16`` (opt-in, honoured only in an fp16
    mode): fp16 MFMA operands with fp32 accumulation, forward and backward."""
    q, k, v, out, lse, d, sfx = _attention_setup(tape, "attention", q, k, v, heads, scale, out, f16)
    return _qkv_attention(tape, "gs_attention", sfx, d, q, k, v, out, lse)


def attention_kv(tape, q, k, v, heads, scale, out=None):
    """Multi-head softmax attention of every pixel of ``q`` [B, Hq, Wq, 64 * heads] to the pixels of ``k`` and
    ``v`` [B, Hk, Wk, 64 * heads] (the Mix Transformer's spatial-reduction attention: k and v come from a
    reduced map; two column slices of one buffer are fine).  fp32 operands in every precision mode (there is
    no fp16-operand form).  No Nq x Nk matrix is stored; the backward's workspace (delta and, where the dK /
    dV kernel splits the queries, the slabs' partials) comes from the pool."""
    q, k, v = materialize(tape, q), materialize(tape, k), materialize(tape, v)
    c = _lib.ATTENTION_HEAD_DIM * heads
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.C != c or t.N != q.N or (name != "q" and (t.H, t.W) != (k.H, k.W)):
            raise ValueError("attention_kv: %s is %s, expected [%d, H, W, %d] for %d heads (k and v of one size)"
                             % (name, tuple(t.t.shape), q.N, c, heads))
    b, nq, nk, dev = q.N, q.H * q.W, k.H * k.W, q.t.device
    if out is None:
        out = Act.empty(b, q.H, q.W, c, dev)
    lse = torch.empty(b * heads * nq, dtype=torch.float32, device=dev)
    d = _lib.attention_kv_desc(b, nq, nk, heads, scale, ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    return _qkv_attention(tape, "gs_attention_kv", "", d, q, k, v, out, lse)


def window_attention(tape, q, k, v, table, heads, ws, shift, scale, out=None):
    """Swin's shifted-window attention, head dimension 32, on padded maps: q, k and v are [B, Hp, Wp, 32 * heads]
    (three column slices of one buffer are fine), Hp and Wp multiples of ``ws``; ``table`` is the max-size
    relative_position_bias_table [(2 ws - 1)^2, heads_max], of which the leading ``heads`` columns are read
    and get a gradient (written like every parameter gradient, then notified).  The roll, the window
    partition, the bias gather and the region mask happen inside the kernel; fp32 operands in every precision
    mode.  lse is kept for the backward, whose workspace (the table partials) comes from the pool."""
    q, k, v = materialize(tape, q), materialize(tape, k), materialize(tape, v)
    c = _lib.WINDOW_ATTENTION_HEAD_DIM * heads
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.C != c or (t.N, t.H, t.W) != (q.N, q.H, q.W):
            raise ValueError("window_attention: %s is %s, expected [%d, %d, %d, %d] for %d heads"
                             % (name, tuple(t.t.shape), q.N, q.H, q.W, c, heads))
    rows = (2 * ws - 1) ** 2
    if table.dim() != 2 or table.shape[0] != rows or table.shape[1] < heads or table.stride(1) != 1:
        raise ValueError("window_attention: the table is %s, expected [%d, >= %d]" % (tuple(table.shape), rows, heads))
    b, dev = q.N, q.t.device
    if out is None:
        out = Act.empty(b, q.H, q.W, c, dev)
    lse = torch.empty(b * heads * q.H * q.W, dtype=torch.float32, device=dev)
    d = _lib.window_attention_desc(b, q.H, q.W, ws, shift, heads, ld_table=table.stride(0), scale=scale, ldq=q.ld,
                                   ldk=k.ld, ldv=v.ld, ldo=out.ld)
    return _qkv_attention(tape, "gs_window_attention", "", d, q, k, v, out, lse, table)


def map_pad(tape, x, hp, wp, out=None):
    """x [B, H, W, C] zero-padded at the bottom and right to [B, hp, wp, C] (Swin pads the normalised map to a
    multiple of the window before the q / k / v linears).  The backward is the crop."""
    L = _L()
    x = materialize(tape, x)
    b, h, w, c, dev = x.N, x.H, x.W, x.C, x.t.device
    if out is None:
        out = Act.empty(b, hp, wp, c, dev)
    _lib.check(L.gs_map_pad(x.ptr, x.ld, out.ptr, out.ld, b, h, w, hp, wp, c, 0, current_stream_ptr()), "gs_map_pad")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        _lib.check(L.gs_map_crop(dy.data_ptr(), dy.stride(2), x.g.data_ptr(), x.g.stride(2), b, h, w, hp, wp, c, acc,
                                 current_stream_ptr()), "gs_map_crop")

    tape.record(backward)
    return out


def map_crop(tape, x, h, w, out=None):
    """the leading [B, h, w, C] of the padded map x [B, Hp, Wp, C].  The backward is the zero-filling pad (added
    where x already holds a gradient)."""
    L = _L()
    x = materialize(tape, x)
    b, hp, wp, c, dev = x.N, x.H, x.W, x.C, x.t.device
    if out is None:
        out = Act.empty(b, h, w, c, dev)
    _lib.check(L.gs_map_crop(x.ptr, x.ld, out.ptr, out.ld, b, h, w, hp, wp, c, 0, current_stream_ptr()),
               "gs_map_crop")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        _lib.check(L.gs_map_pad(dy.data_ptr(), dy.stride(2), x.g.data_ptr(), x.g.stride(2), b, h, w, hp, wp, c, acc,
                                current_stream_ptr()), "gs_map_pad")

    tape.record(backward)
    return out


def cell_layernorm(tape, x, weight, bias, eps=1e-5, out=None):
    """The LayerNorm of Swin's patch merging on the map itself: statistics over the 4 C values of every 2 x 2
    cell of x [B, H, W, C] (H, W even), ``weight`` / ``bias`` the max-size [4 Cmax] parameters in transformers'
    order, read at (2 col + row) * Cmax + c.  The result is a map again: a 2x2 stride-2 convolution is the
    reduction.  The per-cell mean and 1/std are kept for the backward."""
    L = _L()
    x = materialize(tape, x)
    c, cmax = x.C, weight.shape[0] // 4
    if weight.shape[0] % 4 or c > cmax or c % 4 or x.H % 2 or x.W % 2:
        raise ValueError("cell_layernorm: a map %s under parameters of %d entries (needs even sides, C %% 4 == 0 "
                         "and C <= Cmax)" % (tuple(x.t.shape), weight.shape[0]))
    dev, cells = x.t.device, x.N * (x.H // 2) * (x.W // 2)
    if out is None:
        out = Act.empty(x.N, x.H, x.W, c, dev)
    stats = torch.empty(2 * cells, dtype=torch.float32, device=dev)
    mean_ptr, rstd_ptr = stats.data_ptr(), stats.data_ptr() + 4 * cells
    d = _lib.cell_layernorm_desc(x.N, x.H, x.W, c, cmax, eps, ldx=x.ld, ldy=out.ld)
    _lib.check(L.gs_cell_layernorm_forward(ctypes.byref(d), x.ptr, weight.data_ptr(), bias.data_ptr(), out.ptr,
                                           mean_ptr, rstd_ptr, current_stream_ptr()), "gs_cell_layernorm_forward")

    def backward():
        dy = out.g
        if dy is None:
            return
        keep = stats  # noqa: F841 -- the closure owns the storage behind mean_ptr / rstd_ptr
        if dy.stride(2) != d.ldy:
            raise RuntimeError("cell_layernorm: the gradient's pitch %d differs from the output's %d"
                               % (dy.stride(2), d.ldy))
        db = ctypes.byref(d)
        gw, gb = _param_grad(weight), _param_grad(bias)
        ws_buf = _ws.get(L.gs_cell_layernorm_workspace_bytes(db), dev)
        dx, acc = _grad_target(x)
        if dx.stride(2) != d.ldx:   # (an installed gradient of another pitch; scratch has x's)
            raise RuntimeError("cell_layernorm: dx has pitch %d, x has %d" % (dx.stride(2), d.ldx))
        _lib.check(L.gs_cell_layernorm_backward(db, x.ptr, dy.data_ptr(), weight.data_ptr(), mean_ptr, rstd_ptr,
                                                dx.data_ptr(), gw.data_ptr(), gb.data_ptr(), acc, ws_buf.data_ptr(),
                                                ws_buf.numel(), current_stream_ptr()), "gs_cell_layernorm_backward")
        _notify_params(weight, bias)

    tape.record(backward)
    return out


def _forward_only(tape, what, *inputs):
    if tape.enabled and any(t.requires_grad for t in inputs):
        raise NotImplementedError("%s: forward only (no backward kernel); called with a recording tape and an "
                                  "input that requires grad" % what)


def attention_relpos(tape, q, k, v, heads, scale, table, window, out=None, f16=False):
    """BEiT's attention, forward only: ``attention`` with table[idx(i, j), h] added to the scaled score of
    (query i, key j) in head h.  ``table`` is a relative_position_bias_table [(2 Wh - 1)(2 Ww - 1) + 3, heads]
    (fp32, any row pitch), ``window`` = (Wh, Ww), N = Wh * Ww + 1 tokens with the cls token first.  The
    kernel gathers from the table: no N x N bias exists.  ``f16`` as for ``attention``; the bias stays fp32."""
    L = _L()
    _forward_only(tape, "attention_relpos", q, k, v, table)
    q, k, v, out, lse, d, sfx = _attention_setup(tape, "attention_relpos", q, k, v, heads, scale, out, f16)
    wh, ww = window
    rows = (2 * wh - 1) * (2 * ww - 1) + 3
    if table.dim() != 2 or table.shape[0] != rows or table.shape[1] < heads or table.stride(1) != 1:
        raise ValueError("attention_relpos: the table is %s, expected [%d, >= %d] for a %d x %d window"
                         % (tuple(table.shape), rows, heads, wh, ww))
    if rows > _lib.ATTENTION_RELPOS_MAX_ROWS:
        raise ValueError("attention_relpos: a %d x %d window needs %d table rows, the kernel stages at most "
                         "%d in LDS" % (wh, ww, rows, _lib.ATTENTION_RELPOS_MAX_ROWS))
    _lib.check(getattr(L, "gs_attention_relpos_forward" + sfx)(
        ctypes.byref(d), q.ptr, k.ptr, v.ptr, table.data_ptr(), table.stride(0), wh, ww, out.ptr,
        lse.data_ptr(), current_stream_ptr()), "gs_attention_relpos_forward" + sfx)
    return out


def _deconv_packed(weight):
    """torch's ConvTranspose2d weight [Cin, Cout, 2, 2] as the GEMM operand [Cin][2][2][Cout] of
    gs_deconv2x2_forward: made on first use, again when the parameter has been written to (``_version``)
    or moved."""
    key = (weight._version, weight.data_ptr(), weight.device)
    cached = weight.__dict__.get("_gs_deconv_packed")
    if cached is None or cached[0] != key:
        cached = weight._gs_deconv_packed = (key, weight.detach().permute(0, 2, 3, 1).contiguous())
    return cached[1]


def deconv2x2(tape, x, weight, bias, out=None):
    """nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) forward on an NHWC activation; ``weight`` is
    the Parameter in torch's [Cin, Cout, 2, 2] layout.  Forward only."""
    L = _L()
    _forward_only(tape, "deconv2x2", x, weight, *([bias] if bias is not None else []))
    x = materialize(tape, x)
    cin, cout = weight.shape[0], weight.shape[1]
    if tuple(weight.shape[2:]) != (2, 2) or x.C != cin:
        raise ValueError("deconv2x2: weight %s does not fit an input of %d channels (expected [%d, Cout, 2, 2])"
                         % (tuple(weight.shape), x.C, x.C))
    if cin % 4 or cout % 4:
        raise ValueError("deconv2x2 needs channel counts that are multiples of 4, got %d -> %d" % (cin, cout))
    dev = x.t.device
    if out is None:
        out = Act.empty(x.N, 2 * x.H, 2 * x.W, cout, dev)
    w4 = _deconv_packed(weight)
    ws = _ws.get(L.gs_deconv2x2_workspace_bytes(x.N, x.H, x.W, cin, cout), dev)
    _lib.check(L.gs_deconv2x2_forward(x.ptr, x.N, x.H, x.W, cin, x.ld, w4.data_ptr(), cout,
                                      bias.data_ptr() if bias is not None else None, out.ptr, out.ld,
                                      ws.data_ptr(), ws.numel(), current_stream_ptr()), "gs_deconv2x2_forward")
    return out


def vit_tokens(tape, patches, cls_token, pos_embed):
    """ElasticTransformer's token assembly: from the patch embedding [B, Hp, Wp, D] and the max-size
    ``cls_token`` [1, 1, D_max] / ``pos_embed`` [1, N_max, D_max] Parameters, the token activation
    [B, 1, 1 + Hp*Wp, D] with x[b, 0] = cls + pos[0] and x[b, 1 + t] = patch[b, t] + pos[1 + t], on the
    leading D columns and 1 + Hp*Wp rows of the parameters."""
    L = _L()
    patches = materialize(tape, patches)
    b, t, dch, dev = patches.N, patches.H * patches.W, patches.C, patches.t.device
    if dch % 4:
        raise ValueError("vit_tokens needs an embedding width that is a multiple of 4, got %d" % dch)
    if dch > cls_token.shape[-1] or dch > pos_embed.shape[-1] or t + 1 > pos_embed.shape[1]:
        raise ValueError("vit_tokens: %d tokens of width %d exceed pos_embed %s"
                         % (t + 1, dch, tuple(pos_embed.shape)))
    ldpos = pos_embed.stride(1)
    out = Act.empty(b, 1, t + 1, dch, dev)
    _lib.check(L.gs_vit_tokens_forward(patches.ptr, patches.ld, cls_token.data_ptr(), pos_embed.data_ptr(),
                                       ldpos, out.ptr, out.ld, b, t, dch, current_stream_ptr()),
               "gs_vit_tokens_forward")

    def backward():
        dx = out.g
        if dx is None:
            return
        gc, gp = _param_grad(cls_token), _param_grad(pos_embed)
        dp, _ = _grad_target(patches, "patch embedding")
        _lib.check(L.gs_vit_tokens_backward(dx.data_ptr(), dx.stride(2), dp.data_ptr(), dp.stride(2),
                                            gc.data_ptr(), gp.data_ptr(), ldpos, b, t, dch,
                                            current_stream_ptr()), "gs_vit_tokens_backward")
        _notify_params(cls_token, pos_embed)

    tape.record(backward)
    return out


def vit_feature_map(tape, x, hp, wp):
    """The tokens [B, 1, 1 + hp*wp, D] without their cls row as an NHWC feature map [B, hp, wp, D].  An
    activation cannot express the per-image row offset, so the rows are copied (one gs_copy2d per image)."""
    L = _L()
    b, n, c, dev = x.N, x.W, x.C, x.t.device
    if n != 1 + hp * wp:
        raise ValueError("vit_feature_map: %d tokens are not 1 + %d x %d" % (n, hp, wp))
    out = Act.empty(b, hp, wp, c, dev)
    st = current_stream_ptr()
    for i in range(b):
        _lib.check(L.gs_copy2d(x.ptr + 4 * (i * n + 1) * x.ld, x.ld, out.ptr + 4 * i * (n - 1) * out.ld, out.ld,
                               n - 1, c, 1.0, 0, st), "gs_copy2d")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        if not acc:
            x.g.zero_()   # the cls rows receive nothing from this edge
        s = current_stream_ptr()
        g, ldg = x.g, x.g.stride(2)
        for i in range(b):
            _lib.check(L.gs_copy2d(dy.data_ptr() + 4 * i * (n - 1) * dy.stride(2), dy.stride(2),
                                   g.data_ptr() + 4 * (i * n + 1) * ldg, ldg, n - 1, c, 1.0, 1, s), "gs_copy2d")

    tape.record(backward)
    return out


def fcu_tokens(tape, patches, cls_token):
    """ElasticConvformer's token assembly: vit_tokens without a position embedding.  From the patch
    embedding [B, Hp, Wp, D] and the max-size ``cls_token`` [1, 1, D_max] the token activation
    [B, 1, 1 + Hp*Wp, D] with x[b, 0] = cls[:D] and x[b, 1 + t] = patch[b, t]."""
    L = _L()
    patches = materialize(tape, patches)
    b, t, dch, dev = patches.N, patches.H * patches.W, patches.C, patches.t.device
    if dch % 4:
        raise ValueError("fcu_tokens needs an embedding width that is a multiple of 4, got %d" % dch)
    if dch > cls_token.shape[-1]:
        raise ValueError("fcu_tokens: width %d exceeds cls_token %s" % (dch, tuple(cls_token.shape)))
    out = Act.empty(b, 1, t + 1, dch, dev)
    _lib.check(L.gs_fcu_tokens_forward(patches.ptr, patches.ld, cls_token.data_ptr(), out.ptr, out.ld, b, t,
                                       dch, current_stream_ptr()), "gs_fcu_tokens_forward")

    def backward():
        dx = out.g
        if dx is None:
            return
        gc = _param_grad(cls_token)
        dp, _ = _grad_target(patches, "patch embedding")
        _lib.check(L.gs_fcu_tokens_backward(dx.data_ptr(), dx.stride(2), dp.data_ptr(), dp.stride(2),
                                            gc.data_ptr(), b, t, dch, current_stream_ptr()),
                   "gs_fcu_tokens_backward")
        _notify_params(cls_token)

    tape.record(backward)
    return out


def fcu_down(tape, z, x_t, ln):
    """ElasticConvformer's conv-to-token unit behind its pooling and projection, with the add of the token
    stream: from the projected map ``z`` [B, Hc, Wc, D], the tokens ``x_t`` [B, 1, 1 + Hc*Wc, D] and the DynLN
    module ``ln`` (leading D of its parameters),
        out[b, 0] = x_t[b, 0] + x_t[b, 0],   out[b, 1 + t] = x_t[b, 1 + t] + GELU(LN(z[b, t])),
    one kernel (gs_fcu_down_forward).  The backward recomputes the GELU input; x_t has other consumers (its
    gradient accumulates), z has this one."""
    L = _L()
    z, x_t = materialize(tape, z), materialize(tape, x_t)
    weight, bias = ln.weight, ln.bias
    c = _active_width(z, weight, "fcu_down")
    b, t, dev = z.N, z.H * z.W, z.t.device
    if (x_t.N, x_t.H, x_t.W, x_t.C) != (b, 1, t + 1, c):
        raise ValueError("fcu_down: tokens %s do not belong to the map %s"
                         % (tuple(x_t.t.shape), tuple(z.t.shape)))
    out = Act.empty(b, 1, t + 1, c, dev)
    stats = torch.empty(2 * b * t, dtype=torch.float32, device=dev)
    mean_ptr, rstd_ptr = stats.data_ptr(), stats.data_ptr() + 4 * b * t
    d = _lib.fcu_down_desc(b, t, c, ln.eps, ldz=z.ld, ldxt=x_t.ld, ldo=out.ld)
    _lib.check(L.gs_fcu_down_forward(ctypes.byref(d), z.ptr, x_t.ptr, weight.data_ptr(), bias.data_ptr(),
                                     out.ptr, mean_ptr, rstd_ptr, current_stream_ptr()), "gs_fcu_down_forward")

    def backward():
        dout = out.g
        if dout is None:
            return
        keep = stats  # noqa: F841 -- the closure owns the storage behind mean_ptr / rstd_ptr
        gw, gb = _param_grad(weight), _param_grad(bias)
        dz, _ = _grad_target(z, "fcu_down: the projected map")
        dxt, acc = _grad_target(x_t)
        d.ldo, d.lddz, d.lddxt = dout.stride(2), dz.stride(2), dxt.stride(2)
        db = ctypes.byref(d)
        ws = _ws.get(L.gs_fcu_down_workspace_bytes(db), dev)
        _lib.check(L.gs_fcu_down_backward(db, z.ptr, dout.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                          mean_ptr, rstd_ptr, dz.data_ptr(), dxt.data_ptr(), gw.data_ptr(),
                                          gb.data_ptr(), acc, ws.data_ptr(), ws.numel(), current_stream_ptr()),
                   "gs_fcu_down_backward")
        _notify_params(weight, bias)

    tape.record(backward)
    return out


def fcu_up_add(tape, x, r, s):
    """ElasticConvformer's token-to-conv unit behind its projection, with the add in front of the 3x3
    conv: x + nearest_upsample(r, s) for x [B, H, W, C] and r [B, H/s, W/s, C], one kernel.  Both inputs are
    written out first where their BatchNorm was deferred.  The gradient of x is the output's, handed on
    without a copy; r's is the ordered sum over its s x s blocks."""
    L = _L()
    x, r = materialize(tape, x), materialize(tape, r)
    c, dev = x.C, x.t.device
    if s < 1 or (r.N, r.H * s, r.W * s, r.C) != (x.N, x.H, x.W, c):
        raise ValueError("fcu_up_add: %s is not %s upsampled by %s" % (tuple(x.t.shape), tuple(r.t.shape), s))
    if c % 4:
        raise ValueError("fcu_up_add needs a channel count that is a multiple of 4, got %d" % c)
    out = Act.empty(x.N, x.H, x.W, c, dev)
    _lib.check(L.gs_fcu_up_add_forward(x.ptr, r.ptr, out.ptr, x.N, x.H, x.W, c, s, x.ld, r.ld, out.ld,
                                       current_stream_ptr()), "gs_fcu_up_add_forward")

    def backward():
        dout = out.g
        if dout is None:
            return
        st = current_stream_ptr()
        if r.requires_grad:
            acc = _input_grad(r)
            _lib.check(L.gs_fcu_up_add_backward(dout.data_ptr(), r.g.data_ptr(), x.N, x.H, x.W, c, s,
                                                dout.stride(2), r.g.stride(2), acc, st),
                       "gs_fcu_up_add_backward")
        if x.requires_grad:
            _pass_residual_grad(L, x, dout, x.rows, c, st)

    tape.record(backward)
    return out


def ocr_gather(tape, feats, logits, scale=1.0):
    """OCRNet's soft object regions (mmseg's SpatialGatherModule): from the pixel features ``feats``
    [B, H, W, C] (possibly a channel slice of a wider buffer) and the previous head's ``logits`` [B, H, W, K]
        w = softmax over the H*W pixels of scale * logits[..., k],   context[b, k] = sum_p w[b, k, p] feats[b, p]
    as a K x 1 map [B, K, 1, C] (gs_ocr_gather_forward; w is never stored, the statistics of every class
    map are kept for the backward).  The features have other consumers (their gradient accumulates); the
    logits have this one inside the node.  The scratch (one [K, C] partial per 128 pixels) lies far inside
    what reserve_workspaces sets aside."""
    L = _L()
    feats, logits = materialize(tape, feats), materialize(tape, logits)
    b, p, k, c, dev = feats.N, feats.H * feats.W, logits.C, feats.C, feats.t.device
    if (logits.N, logits.H, logits.W) != (b, feats.H, feats.W):
        raise ValueError("ocr_gather: logits %s and features %s differ in size"
                         % (tuple(logits.t.shape), tuple(feats.t.shape)))
    if c % 4:
        raise ValueError("ocr_gather needs a channel count that is a multiple of 4, got %d" % c)
    out = Act.empty(b, k, 1, c, dev)
    stats = torch.empty(2 * b * k, dtype=torch.float32, device=dev)
    d = _lib.ocr_gather_desc(b, p, k, c, scale, ldl=logits.ld, ldf=feats.ld, ldc=out.ld)
    db = ctypes.byref(d)
    ws = _ws.get(L.gs_ocr_gather_workspace_bytes(db), dev)
    _lib.check(L.gs_ocr_gather_forward(db, logits.ptr, feats.ptr, out.ptr, stats.data_ptr(), ws.data_ptr(),
                                       ws.numel(), current_stream_ptr()), "gs_ocr_gather_forward")

    def backward():
        dctx = out.g
        if dctx is None:
            return
        dl, _ = _grad_target(logits, "ocr_gather: the logits map")
        df, acc = _grad_target(feats)
        d.lddl, d.lddf, d.lddc = dl.stride(2), df.stride(2), dctx.stride(2)
        wsb = _ws.get(L.gs_ocr_gather_workspace_bytes(db), dev)
        _lib.check(L.gs_ocr_gather_backward(db, logits.ptr, feats.ptr, out.ptr, stats.data_ptr(),
                                            dctx.data_ptr(), dl.data_ptr(), df.data_ptr(), acc, wsb.data_ptr(),
                                            wsb.numel(), current_stream_ptr()), "gs_ocr_gather_backward")

    tape.record(backward)
    return out


def ocr_attend(tape, q, k, v):
    """OCRNet's pixel-to-region attention (the core of mmseg's ObjectAttentionBlock): queries ``q``
    [B, H, W, ch], keys and values ``k``, ``v`` [B, K, 1, ch] (region maps),
        out[b, p] = sum_k softmax_k(ch^-0.5 <q[b, p], k[b, k]>) v[b, k],
    one kernel (gs_ocr_attend_forward).  The [B, H*W, K] map is not kept: the backward recomputes it from
    q, k and the saved log-sum-exp of every pixel.  Each input has this one consumer."""
    L = _L()
    q, k, v = materialize(tape, q), materialize(tape, k), materialize(tape, v)
    b, p, ch, dev = q.N, q.H * q.W, q.C, q.t.device
    kk = k.H * k.W
    if (k.N, k.C) != (b, ch) or (v.N, v.H, v.W, v.C) != (b, k.H, k.W, ch):
        raise ValueError("ocr_attend: queries %s, keys %s and values %s do not belong together"
                         % (tuple(q.t.shape), tuple(k.t.shape), tuple(v.t.shape)))
    if ch % 4:
        raise ValueError("ocr_attend needs a channel count that is a multiple of 4, got %d" % ch)
    out = Act.empty(b, q.H, q.W, ch, dev)
    lse = torch.empty(b * p, dtype=torch.float32, device=dev)
    d = _lib.ocr_attend_desc(b, p, kk, ch, ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    _lib.check(L.gs_ocr_attend_forward(ctypes.byref(d), q.ptr, k.ptr, v.ptr, out.ptr, lse.data_ptr(),
                                       current_stream_ptr()), "gs_ocr_attend_forward")

    def backward():
        dout = out.g
        if dout is None:
            return
        dq, _ = _grad_target(q, "ocr_attend: the query map")
        dk, _ = _grad_target(k, "ocr_attend: the key map")
        dv, _ = _grad_target(v, "ocr_attend: the value map")
        d.lddq, d.lddk, d.lddv, d.lddo = dq.stride(2), dk.stride(2), dv.stride(2), dout.stride(2)
        db = ctypes.byref(d)
        ws = _ws.get(L.gs_ocr_attend_workspace_bytes(db), dev)
        _lib.check(L.gs_ocr_attend_backward(db, q.ptr, k.ptr, v.ptr, out.ptr, lse.data_ptr(), dout.data_ptr(),
                                            dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(),
                                            ws.numel(), current_stream_ptr()), "gs_ocr_attend_backward")

    tape.record(backward)
    return out


def _pass_residual_grad(L, residual, src, rows, C, stream):
    """Hand the gradient ``src`` of an identity edge to ``residual``: aliased as residual.g when it
    is the first contribution and the layouts match, else copied (added where residual.g holds a
    contribution)."""
    if residual.g is None and residual.parent is None and src.stride() == residual.t.stride():
        residual.g = src
        return
    acc = _input_grad(residual)
    _lib.check(L.gs_copy2d(src.data_ptr(), src.stride(2), residual.g.data_ptr(),
                           residual.g.stride(2), rows, C, 1.0, acc, stream), "gs_copy2d")


class BNParams:
    """What the BN kernels need from a DynBN / SyncBN module (leading-slice semantics, A2)."""
    __slots__ = ("weight", "bias", "running_mean", "running_var", "eps", "momentum", "training",
                 "process_group", "num_batches_tracked")

    def __init__(self, weight, bias, running_mean, running_var, eps, momentum, training,
                 process_group=None, num_batches_tracked=None):
        self.weight, self.bias = weight, bias
        self.running_mean, self.running_var = running_mean, running_var
        self.eps, self.momentum, self.training = eps, momentum, training
        self.process_group = process_group
        self.num_batches_tracked = num_batches_tracked


def _sync_stats(sums, count, C, pg, equal_counts=False):
    """SyncBN: merge per-rank (shifted sums, count) into global statistics (Chan et al.).

    Mirrors torch.nn.SyncBatchNorm's all_gather of [mean, var, count]; the
    payload is 2C+1 floats per rank."""
    import torch.distributed as dist
    world = dist.get_world_size(pg)
    if sums.is_cuda and equal_counts:
        # device path of the training step: two launches around one all_gather
        L = _L()
        st = current_stream_ptr()
        local = torch.empty(2 * C + 1, dtype=torch.float64, device=sums.device)
        _lib.check(L.gs_bn_sync_local(sums.data_ptr(), float(count), C, local.data_ptr(), st),
                   "gs_bn_sync_local")
        gathered = torch.empty((world, 2 * C + 1), dtype=torch.float64, device=sums.device)
        if dist.get_backend(pg) == "nccl":
            dist.all_gather_into_tensor(gathered, local, group=pg)
        else:   # gloo (tests, rehearsals): list form, rows of `gathered` as outputs
            dist.all_gather([gathered[r] for r in range(world)], local, group=pg)
        merged = torch.empty(3 * C, dtype=torch.float32, device=sums.device)
        _lib.check(L.gs_bn_sync_merge(gathered.data_ptr(), world, C, merged.data_ptr(), st),
                   "gs_bn_sync_merge")
        return merged, float(count) * world
    d1 = sums[:C].double() / count
    mean = sums[2 * C:3 * C].double() + d1
    var = (sums[C:2 * C].double() / count - d1 * d1).clamp_(min=0)
    # (torch.full, not torch.tensor([...], device=...): a host-to-device copy from pageable memory
    # synchronises the stream and would stall the host once per SyncBN layer and step)
    local = torch.cat([mean, var, torch.full((1,), float(count), dtype=torch.float64,
                                             device=sums.device)])
    gathered = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(gathered, local, group=pg)
    g = torch.stack(gathered)                     # [world, 2C+1]
    cnt = g[:, 2 * C:]                            # [world, 1]
    total = cnt.sum()
    gmean = (g[:, :C] * cnt).sum(0) / total
    gvar = ((g[:, C:2 * C] + (g[:, :C] - gmean) ** 2) * cnt).sum(0) / total
    merged = torch.empty_like(sums)
    merged[:C] = 0
    merged[C:2 * C] = (gvar * total).float()
    merged[2 * C:3 * C] = gmean.float()
    if not equal_counts:
        return merged, float(total.item())   # exact for any per-rank counts; synchronises the host
    # equal_counts: every rank holds the same batch and crop size (the training path: fixed
    # samples_per_gpu and crop), so the total is count * world and is NOT read back from the device
    # -- a .item() here drains the GPU queue once per SyncBN layer and step, which serialises host
    # and GPU in multi-GPU runs.  (The weighting of the per-rank statistics above uses the
    # gathered counts either way.)
    return merged, float(count) * world


def batchnorm(tape, x, bn, relu=False, residual=None, out=None, inplace=False):
    """y = act(BN(x) (+ residual)).  Training: batch statistics over N*H*W of the active slice,
    running statistics updated on the slice; eval: running statistics.  ``inplace`` reuses x's
    storage for y (only when x is not needed by backward, i.e. never in training)."""
    L = _L()
    x = materialize(tape, x)
    residual = materialize_residual(tape, residual)
    dev = x.t.device
    C, rows = x.C, x.rows
    st = current_stream_ptr()
    buf = torch.empty(7 * C, dtype=torch.float32, device=dev)   # {sums[3C], coeffs[4C]}
    sums_ptr = buf.data_ptr()
    coeffs_ptr = sums_ptr + 12 * C
    gamma = bn.weight.data_ptr() if bn.weight is not None else None
    beta = bn.bias.data_ptr() if bn.bias is not None else None
    count = float(rows)
    use_batch = bn.training or bn.running_mean is None
    if use_batch:
        if rows <= 1 and bn.process_group is None:
            raise ValueError("Expected more than 1 value per channel when training, got input "
                             "size %s" % (tuple(x.t.shape),))
        nb = L.gs_bn_stats_workspace_bytes(rows, C)
        ws = _ws.get(nb, dev)
        rm = bn.running_mean.data_ptr() if (bn.running_mean is not None and bn.training) else None
        rv = bn.running_var.data_ptr() if (bn.running_var is not None and bn.training) else None
        mom = bn.momentum if bn.momentum is not None else 0.1
        if bn.process_group is None:
            # rank-local statistics: partial sums + (sum, finalize) in two launches
            _lib.check(L.gs_bn_stats_finalize(x.ptr, rows, C, x.ld, gamma, beta, bn.eps, mom, rm, rv,
                                              coeffs_ptr, ws.data_ptr(), ws.numel(), st),
                       "gs_bn_stats_finalize")
        else:
            _lib.check(L.gs_bn_stats(x.ptr, rows, C, x.ld, sums_ptr, ws.data_ptr(),
                                     ws.numel(), st), "gs_bn_stats")
            merged, count = _sync_stats(buf[:3 * C], count, C, bn.process_group, equal_counts=True)
            _lib.check(L.gs_bn_finalize(merged.data_ptr(), count, C, gamma, beta, bn.eps, mom, rm,
                                        rv, coeffs_ptr, st), "gs_bn_finalize")
        if bn.training and bn.num_batches_tracked is not None:
            bn.num_batches_tracked()  # host-side counter: no device op per BN per step
    else:
        _lib.check(L.gs_bn_eval_coeffs(bn.running_mean.data_ptr(), bn.running_var.data_ptr(), C,
                                       gamma, beta, bn.eps, coeffs_ptr, st),
                   "gs_bn_eval_coeffs")
    if out is None:
        out = x if (inplace and not tape.enabled) else Act.empty(x.N, x.H, x.W, C, dev)
    _lib.check(L.gs_bn_apply(x.ptr, rows, C, x.ld, coeffs_ptr,
                             residual.ptr if residual is not None else None,
                             residual.ld if residual is not None else 0, 1 if relu else 0,
                             out.ptr, out.ld, st), "gs_bn_apply")
    if relu:
        _trace_relu(bn, out)

    def backward():
        dy = out.g
        if dy is None:
            return
        s = current_stream_ptr()
        keep = buf  # noqa: F841 -- the closure owns the coefficient storage behind coeffs_ptr
        mask = 0 if not relu else (2 if residual is not None else 1)
        nbw = L.gs_bn_bwd_workspace_bytes(rows, C)
        wsb = _ws.get(nbw, dev)
        bsums = torch.empty(2 * C, dtype=torch.float32, device=dev)
        # the masked gradient g is also the gradient of the identity branch: write it in place
        want_g = residual is not None and residual.requires_grad and relu
        _lib.check(L.gs_bn_bwd_reduce(dy.data_ptr(), dy.stride(2),
                                      x.ptr, x.ld, out.ptr, out.ld, rows, C, coeffs_ptr,
                                      mask, dy.data_ptr() if want_g else None, dy.stride(2),
                                      bsums.data_ptr(), wsb.data_ptr(), wsb.numel(), s),
                   "gs_bn_bwd_reduce")
        bcount = count
        wgrad = bn.weight is not None and bn.weight.requires_grad
        bgrad = bn.bias is not None and bn.bias.requires_grad
        gw = ensure_grad(bn.weight) if wgrad else None
        gb = ensure_grad(bn.bias) if bgrad else None
        synced = use_batch and bn.process_group is not None
        if synced:
            # dx needs the GROUP sums (torch.nn.SyncBatchNorm backward); dgamma / dbeta are this
            # rank's own sums -- the data-parallel gradient all-reduce adds the ranks up afterwards.
            # Writing the group sums there would count every rank world_size times.
            import torch.distributed as dist
            if wgrad:
                gw[:C].copy_(bsums[C:2 * C])
            if bgrad:
                gb[:C].copy_(bsums[:C])
            dist.all_reduce(bsums, group=bn.process_group)
        mask_apply = 0 if want_g else mask  # dy already masked in place
        dx = _sole_grad(x, "BN input")
        _lib.check(L.gs_bn_bwd_apply(dy.data_ptr(), dy.stride(2), x.ptr, x.ld, out.ptr, out.ld,
                                     rows, C, coeffs_ptr, bsums.data_ptr(), bcount,
                                     mask_apply, 1 if use_batch else 0, dx.data_ptr(),
                                     dx.stride(2), gw.data_ptr() if (wgrad and not synced) else None,
                                     gb.data_ptr() if (bgrad and not synced) else None, s),
                   "gs_bn_bwd_apply")
        _notify_params(bn.weight, bn.bias)
        if residual is not None and residual.requires_grad:
            # dy: the masked (relu) or plain (no relu) upstream gradient
            _pass_residual_grad(L, residual, dy, rows, C, s)

    tape.record(backward)
    return out


BNBWD_FUSE = os.environ.get("GS_NO_BNBWD_FUSE") is None
RELU_MASK_BYTES = os.environ.get("GS_RELU_MASK_BYTES", "1") != "0"   # gs_bn_bwd_fuse mode 3
BNBWD_FUSED_COUNT = 0   # diagnostics: how many BN-backward reductions ran inside a dgrad epilogue
BNBWD_FUSED_MASK_COUNT = 0   # ... of which took their ReLU mask from the mask bytes (mode 3)


class _ConvBnPlan:
    """Everything about one conv + BN layer call that depends only on the layer and on the geometry
    of its input: the descriptor, the BN argument block, sizes.  Cached on the weight Parameter per
    (input geometry, active widths, flags): a supernet layer sees a handful of them, and building
    the two ctypes structures was a third of the host time of a layer call.  Pointers (the input's
    deferred-BN coefficients, the BN parameters — an arena rebuild moves them) are NOT part of the
    plan: they are written into the cached structures at every use, forward and backward."""
    __slots__ = ("d", "args", "need", "n", "ho", "wo", "rows", "C", "use_batch", "affine_ok")


def _conv_bn_plan(L, x, weight, co_eff, bn, stride, pad, dil, relu, tag, use_batch):
    kh, kw = weight.shape[2], weight.shape[3]
    if x.nchw_image:
        n, _, h, w = x.t.shape
    else:
        n, h, w = x.N, x.H, x.W
    pl = _ConvBnPlan()
    pl.n = n
    pl.ho, pl.wo = conv_out_size(h, kh, stride, pad, dil), conv_out_size(w, kw, stride, pad, dil)
    pl.rows = n * pl.ho * pl.wo
    pl.C = co_eff
    pl.use_batch = use_batch
    pl.d = d = _conv_desc(x, weight, co_eff, stride, pad, dil, round_up(co_eff, 4),
                          role=1 if tag == "k3" else 0)
    pl.affine_ok = bool(L.gs_conv2d_in_affine_supported(ctypes.byref(d)))
    pl.need = L.gs_conv_bn_workspace_bytes(ctypes.byref(d))
    pl.args = args = _lib.BnArgs()
    args.eps = bn.eps
    args.momentum = bn.momentum if bn.momentum is not None else 0.1
    args.use_batch_stats = 1 if use_batch else 0
    args.update_running = 1 if (bn.training and bn.running_mean is not None) else 0
    args.relu = 1 if relu else 0
    return pl


def _bn_pointers(args, bn):
    w, b, rm, rv = bn.weight, bn.bias, bn.running_mean, bn.running_var
    args.gamma = w.data_ptr() if w is not None else None
    args.beta = b.data_ptr() if b is not None else None
    args.running_mean = rm.data_ptr() if rm is not None else None
    args.running_var = rv.data_ptr() if rv is not None else None


def conv_bn(tape, x, weight, co, bn, stride=1, pad=0, dil=1, relu=False, residual=None, out=None,
            tag=None, defer=False, owns_input_grad=False, defer_residual=False):
    """z = act(BN(conv(x, weight[:co, :x.C])) (+ residual)) through ONE library call per direction
    (gs_conv_bn_forward / gs_conv_bn_backward): same kernels, same results as conv2d() followed by
    batchnorm(), a third of the host work.  Rank-local BatchNorm only (``bn.process_group`` None);
    the conv has no bias.

    ``defer`` (with relu, no residual, no ``out``): the BN + ReLU is NOT applied here; the returned
    activation carries the coefficients (Act.affine) and its consumer — the next conv_bn — evaluates
    relu(bn(y)) in its operand loaders, forward and weight gradient (gs_conv_desc.in_affine).  A
    deferred INPUT ``x`` is consumed that way when the library supports the shape, else written out.

    ``defer_residual`` (no relu, no residual, no ``out``): likewise the BN is not applied; the returned
    activation (the raw conv output) carries the coefficients in ``Act.res_affine`` and must be used
    as the ``residual`` of a conv_bn call, whose apply pass adds bn(residual)
    (gs_bn_args.residual_coeffs).  A ``residual`` that carries ``res_affine`` is consumed that way.

    ``owns_input_grad``: this conv's data gradient is the LAST contribution to ``x.g`` (accumulation
    included).  If x came out of a training-mode BN + ReLU (``x.bnb``), the dgrad epilogue then also
    applies that ReLU's mask and reduces that BN's backward sums (gs_bn_bwd_fuse): the producer's
    backward finds them in ``x.bnb_sums`` and skips its reduction pass over dz and y."""
    _check_precision(tape)
    L = _L()
    co_eff = round_up(co, 4)
    if co_eff != co:   # channel counts that are not multiples of 4 keep the two-step path
        raise ValueError("conv_bn needs an output width that is a multiple of 4, got %d" % co)
    dev = x.t.device
    defer = bool(defer and DEFER_BN and relu and residual is None and out is None)
    defer_residual = bool(defer_residual and DEFER_BN and not relu and residual is None and out is None)
    use_batch = bn.training or bn.running_mean is None
    plans = weight.__dict__.get("_gs_plans")
    if plans is None:
        plans = weight._gs_plans = {}
    pl = None
    for _ in range(2):   # (second round: the deferred input had to be written out)
        key = None if x.nchw_image else (x.N, x.H, x.W, x.C, x.ld, stride, pad, dil, co, relu, tag,
                                         bn.training, use_batch, bn.momentum, bn.eps)
        pl = plans.get(key) if key is not None else None
        if pl is None:
            pl = _conv_bn_plan(L, x, weight, co_eff, bn, stride, pad, dil, relu, tag, use_batch)
            if key is not None:
                if len(plans) > 64:
                    plans.clear()
                plans[key] = pl
        if x.affine is None or pl.affine_ok:
            break
        x = materialize(tape, x)
    if use_batch and pl.rows <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                         % ((pl.n, co, pl.ho, pl.wo),))
    d, args, need, C, rows = pl.d, pl.args, pl.need, pl.C, pl.rows
    y = Act.empty(pl.n, pl.ho, pl.wo, co, dev)
    in_affine = x.affine   # kept alive by the backward closure
    d.in_affine = in_affine.data_ptr() if in_affine is not None else None
    if defer or defer_residual:
        out = y
    elif out is None:
        out = Act.empty(pl.n, pl.ho, pl.wo, co, dev)
    _bn_pointers(args, bn)
    res_affine = residual.res_affine if residual is not None else None   # (kept alive by the closure)
    args.residual_coeffs = res_affine.data_ptr() if res_affine is not None else None
    # A block output relu(bn(y) + identity) whose consumer may fold this BatchNorm's backward
    # reduction into its data-gradient epilogue: the apply pass also writes the ReLU mask as one byte
    # per channel quad, so that epilogue reads rows * C / 4 bytes instead of the activation again
    relu_mask = None
    if (RELU_MASK_BYTES and relu and residual is not None and not defer and use_batch and BNBWD_FUSE
            and tape.enabled and out.parent is None):
        relu_mask = torch.empty((rows, C // 4), dtype=torch.uint8, device=dev)
    args.relu_mask = relu_mask.data_ptr() if relu_mask is not None else None
    # [scale | beta | mean | invstd][C] + a 2C slot for this BatchNorm's backward sums (filled by
    # this layer's backward, or by its consumer's dgrad epilogue): one small allocation per layer
    coeffs = torch.empty(6 * C, dtype=torch.float32, device=dev)
    ws = _ws.get(need, dev)
    _lib.check(L.gs_conv_bn_forward(ctypes.byref(d), x.ptr, weight.data_ptr(), ctypes.byref(args),
                                    residual.ptr if residual is not None else None,
                                    residual.ld if residual is not None else 0, y.ptr,
                                    coeffs.data_ptr(), None if (defer or defer_residual) else out.ptr,
                                    out.ld, ws.data_ptr(), ws.numel(), current_stream_ptr()),
               "gs_conv_bn_forward")
    if use_batch and bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked()
    if defer:
        out.affine = coeffs
        _trace_relu_deferred(bn, y, coeffs)
    elif defer_residual:
        out.res_affine = coeffs
    elif relu:
        _trace_relu(bn, out)
    if relu and use_batch and BNBWD_FUSE and tape.enabled and out.parent is None:
        # (y, coefficients, mask mode).  Mode 2 masks with the post-activation output, i.e. with the
        # activation that carries this tuple: it is NOT stored in the tuple — a self-reference would
        # make every residual output an uncollectable-by-refcount cycle, its device memory would
        # live until Python's cyclic GC happens to run, and the caching allocator would answer with
        # ~15 hipMalloc calls per step (measured: reserved memory 7.7 -> 25 GB over 60 steps)
        # Likewise a deferred output IS its BN input y: stored as None, the consumer substitutes x.
        # (mode 3: the mask bytes written above stand in for the activation of mode 2)
        out.bnb = (None if out is y else y, coeffs,
                   3 if relu_mask is not None else (2 if residual is not None else 1), relu_mask)
    x_bnb = x.bnb if (owns_input_grad and BNBWD_FUSE and x.requires_grad) else None
    if not tape.enabled:
        return out

    def backward():
        dz = out.g
        if dz is None:
            return
        s = current_stream_ptr()
        mask = 0 if not relu else (2 if residual is not None else 1)
        sums_ready = out.bnb_sums is not None    # a consumer's dgrad epilogue did the reduction
        want_g = residual is not None and residual.requires_grad and relu
        wgrad_bn = bn.weight is not None and bn.weight.requires_grad
        bgrad_bn = bn.bias is not None and bn.bias.requires_grad
        ggamma = ensure_grad(bn.weight) if wgrad_bn else None
        gbeta = ensure_grad(bn.bias) if bgrad_bn else None
        gw = ensure_grad(weight) if weight.requires_grad else None
        dy = torch.empty_like(y.t)
        bsums_ptr = coeffs.data_ptr() + 16 * C
        acc = 0
        dx_ptr = None
        if x.requires_grad:
            acc = _input_grad(x)
            dx_ptr = x.g.data_ptr()
        fuse, fused_flag = None, None
        if x_bnb is not None and dx_ptr is not None and x.parent is None:
            py, pcoeffs, pmode, pmask = x_bnb
            if py is None:
                py = x
            pact = x if pmode == 2 else None
            fused_flag = ctypes.c_int32(0)
            fuse = _lib.BnBwdFuse()
            fuse.y, fuse.ldy = py.ptr, py.ld
            fuse.act, fuse.ldact = (pact.ptr, pact.ld) if pact is not None else (None, 0)
            pc = pcoeffs.data_ptr()
            fuse.coeffs, fuse.sums = pc, pc + 16 * (pcoeffs.numel() // 6)   # the producer's sums slot
            fuse.fused = ctypes.pointer(fused_flag)
            fuse.mode, fuse.reserved = pmode, 0
            fuse.mask, fuse.ldmask, fuse.reserved2 = (
                (pmask.data_ptr(), pmask.shape[1], 0) if pmode == 3 else (None, 0, 0))
        ws_b = _ws.get(need, dev)
        queued = SIDE_WGRAD and gw is not None
        d.in_affine = in_affine.data_ptr() if in_affine is not None else None
        _bn_pointers(args, bn)
        _lib.check(L.gs_conv_bn_backward(
            ctypes.byref(d), x.ptr, weight.data_ptr(), y.ptr, out.ptr, out.ld, coeffs.data_ptr(),
            ctypes.byref(args), dz.data_ptr(), dz.stride(2), mask, 1 if want_g else 0,
            dy.data_ptr(), bsums_ptr, ggamma.data_ptr() if wgrad_bn else None,
            gbeta.data_ptr() if bgrad_bn else None,
            gw.data_ptr() if (gw is not None and not queued) else None,
            dx_ptr, acc, ws_b.data_ptr(), ws_b.numel(), None, 0, s, None,
            ctypes.byref(fuse) if fuse is not None else None, 1 if sums_ready else 0),
            "gs_conv_bn_backward")
        if fuse is not None and fused_flag.value:
            global BNBWD_FUSED_COUNT, BNBWD_FUSED_MASK_COUNT
            BNBWD_FUSED_COUNT += 1
            if fuse.mode == 3:
                BNBWD_FUSED_MASK_COUNT += 1
            x.bnb_sums = True        # x.g now holds the MASKED gradient of the producer's ReLU
        _notify_params(bn.weight, bn.bias)
        if queued:
            _streams.queue_wgrad(d, x, dy, weight, gw, need, dev)     # the side stream gets it in a batch
        elif gw is not None:
            _notify(weight)
        if residual is not None and residual.requires_grad:
            # dz: the masked (relu) or plain (no relu) upstream gradient
            _pass_residual_grad(L, residual, dz, rows, C, s)

    tape.record(backward)
    return out


def maxpool(tape, x, k=3, s=2, p=1):
    L = _L()
    dev = x.t.device
    ho, wo = (x.H + 2 * p - k) // s + 1, (x.W + 2 * p - k) // s + 1
    out = Act.empty(x.N, ho, wo, x.C, dev)
    idx = torch.empty((x.N, ho, wo, x.C), dtype=torch.uint8, device=dev)
    _lib.check(L.gs_maxpool_forward(x.ptr, x.N, x.H, x.W, x.C, x.ld, k, s, p, ho, wo, out.ptr,
                                    out.ld, idx.data_ptr(), current_stream_ptr()),
               "gs_maxpool_forward")
    if POOL_TRACE is not None:
        POOL_TRACE.append(idx)

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        _lib.check(L.gs_maxpool_backward(dy.data_ptr(), dy.stride(2), idx.data_ptr(), x.N, x.H, x.W,
                                         x.C, k, s, p, ho, wo, x.g.data_ptr(), x.g.stride(2),
                                         acc, current_stream_ptr()),
                   "gs_maxpool_backward")

    tape.record(backward)
    return out


def avgpool_ceil(tape, x, s):
    """nn.AvgPool2d(s, stride=s, ceil_mode=True, count_include_pad=False) (avg_down shortcut)."""
    L = _L()
    x = materialize(tape, x)
    dev = x.t.device
    ho, wo = (x.H + s - 1) // s, (x.W + s - 1) // s
    out = Act.empty(x.N, ho, wo, x.C, dev)
    _lib.check(L.gs_avgpool_ceil_forward(x.ptr, x.N, x.H, x.W, x.C, x.ld, s, out.ptr, out.ld,
                                         current_stream_ptr()), "gs_avgpool_ceil_forward")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        _lib.check(L.gs_avgpool_ceil_backward(dy.data_ptr(), dy.stride(2), x.N, x.H, x.W, x.C, s,
                                              x.g.data_ptr(), x.g.stride(2), acc,
                                              current_stream_ptr()), "gs_avgpool_ceil_backward")

    tape.record(backward)
    return out


def copy_into(tape, x, dst):
    """dst[..., :x.C] = x  (first member of a fused concat)."""
    L = _L()
    _lib.check(L.gs_copy2d(x.ptr, x.ld, dst.ptr, dst.ld, x.rows, x.C, 1.0, 0, current_stream_ptr()),
               "gs_copy2d")

    def backward():
        dg = dst.g
        if dg is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        _lib.check(L.gs_copy2d(dg.data_ptr(), dg.stride(2), x.g.data_ptr(), x.g.stride(2), x.rows,
                               x.C, 1.0, acc, current_stream_ptr()), "gs_copy2d")

    tape.record(backward)
    return dst


def adaptive_avgpool(tape, x, scales):
    """All PPM pool scales in one read of x. Returns one Act [N,s,s,C] per scale."""
    L = _L()
    dev = x.t.device
    ns = len(scales)
    arr = _int32_array(ns)(*scales)
    total_bins = sum(s * s for s in scales)
    ybuf = torch.empty(x.N * total_bins * x.C, dtype=torch.float32, device=dev)
    nb = L.gs_adaptive_avgpool_workspace_bytes(x.N, x.H, x.W, x.C, arr, ns)
    ws = _ws.get(nb, dev)
    _lib.check(L.gs_adaptive_avgpool_forward(x.ptr, x.N, x.H, x.W, x.C, x.ld, arr, ns,
                                             ybuf.data_ptr(), ws.data_ptr(), ws.numel(),
                                             current_stream_ptr()), "gs_adaptive_avgpool_forward")
    outs, off = [], 0
    for s in scales:
        n_el = x.N * s * s * x.C
        outs.append(Act(ybuf[off:off + n_el].view(x.N, s, s, x.C)))
        off += n_el

    def backward():
        if not x.requires_grad:
            return
        if all(o.g is None for o in outs):
            return
        gbuf = torch.zeros_like(ybuf)
        off2 = 0
        for s, o in zip(scales, outs):
            n_el = x.N * s * s * x.C
            if o.g is not None:
                gbuf[off2:off2 + n_el].view(x.N, s, s, x.C).copy_(o.g)
            off2 += n_el
        acc = _input_grad(x)
        _lib.check(L.gs_adaptive_avgpool_backward(gbuf.data_ptr(), x.N, x.H, x.W, x.C, arr, ns,
                                                  x.g.data_ptr(), x.g.stride(2), acc,
                                                  current_stream_ptr()),
                   "gs_adaptive_avgpool_backward")

    tape.record(backward)
    return outs


def bilinear(tape, x, size, align_corners=False, out=None, accumulate=False):
    """mmseg.ops.resize(mode='bilinear').  ``out`` may be a channel slice of a concat buffer;
    ``accumulate`` adds into ``out`` (UPer top-down path)."""
    L = _L()
    dev = x.t.device
    ho, wo = int(size[0]), int(size[1])
    if out is None:
        out = Act.empty(x.N, ho, wo, x.C, dev)
    al = 1 if align_corners else 0
    _lib.check(L.gs_bilinear_forward(x.ptr, x.N, x.H, x.W, x.C, x.ld, ho, wo, al, out.ptr, out.ld,
                                     1 if accumulate else 0, current_stream_ptr()),
               "gs_bilinear_forward")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        acc = _input_grad(x)
        nb = L.gs_bilinear_backward_workspace_bytes(x.N, x.H, x.W, x.C, ho, wo)
        ws = _ws.get(nb, dev)
        _lib.check(L.gs_bilinear_backward(dy.data_ptr(), dy.stride(2), x.N, x.H, x.W, x.C, ho, wo,
                                          al, x.g.data_ptr(), x.g.stride(2), acc,
                                          ws.data_ptr(), ws.numel(), current_stream_ptr()),
                   "gs_bilinear_backward")

    tape.record(backward)
    return out


def dropout2d(tape, x, p, training, generator=None):
    """nn.Dropout2d: one Bernoulli(1-p) draw per (n, channel), scaled by 1/(1-p)."""
    if not training or p <= 0.0:
        return x
    L = _L()
    dev = x.t.device
    keep = 1.0 - p
    mask = torch.empty((x.N, x.C), dtype=torch.float32, device=dev)
    mask.bernoulli_(keep, generator=generator).div_(keep)
    out = Act.empty(x.N, x.H, x.W, x.C, dev)
    ppi = x.H * x.W
    _lib.check(L.gs_scale_nc(x.ptr, x.ld, mask.data_ptr(), x.N, ppi, x.C, out.ptr, out.ld,
                             current_stream_ptr()), "gs_scale_nc")

    def backward():
        dy = out.g
        if dy is None or not x.requires_grad:
            return
        dx = _sole_grad(x, "dropout input")
        _lib.check(L.gs_scale_nc(dy.data_ptr(), dy.stride(2), mask.data_ptr(), x.N, ppi, x.C,
                                 dx.data_ptr(), dx.stride(2), current_stream_ptr()), "gs_scale_nc")

    tape.record(backward)
    return out


def add_grad_passthrough(tape, src, dst):
    """Record that ``dst`` is the same values as ``src`` (identity edge): route dst.g into src.g."""
    L = _L()

    def backward():
        dg = dst.g
        if dg is None or not src.requires_grad:
            return
        _pass_residual_grad(L, src, dg, src.rows, src.C, current_stream_ptr())

    tape.record(backward)


# diagnostics for the tests only (like BNBWD_FUSED_COUNT): gs_batch_rescale launches batch_rescale
# has made; nothing in the package reads it
BATCH_RESCALE_CALLS = 0


def batch_rescale(img, gt, size):
    """A normalised batch at another resolution (data.input_shape): ``img``
    fp32 NCHW [N,3,h,w] bilinear (align_corners=False), ``gt`` int64 [N,1,h,w] nearest or None, both
    in ONE gs_batch_rescale launch on the current stream.  ``size`` = (H, W); a size equal to (h, w)
    returns the inputs themselves without a launch.  Returns (img, gt) as new tensors."""
    global BATCH_RESCALE_CALLS
    H, W = int(size[0]), int(size[1])
    if not img.is_cuda or (gt is not None and not gt.is_cuda):
        raise _lib.HipLibraryError("batch_rescale needs device tensors (no CPU fallback)")
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
        raise ValueError("batch_rescale: img must be fp32 [N,3,h,w], got %s %s"
                         % (img.dtype, tuple(img.shape)))
    n, _, h, w = img.shape
    if gt is not None and (gt.dtype != torch.int64 or tuple(gt.shape) != (n, 1, h, w)):
        raise ValueError("batch_rescale: gt_semantic_seg must be int64 [%d,1,%d,%d], got %s %s"
                         % (n, h, w, gt.dtype, tuple(gt.shape)))
    if (H, W) == (h, w):
        return img, gt
    img = img.contiguous()
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=img.device)
    out_gt = None
    if gt is not None:
        gt = gt.contiguous()
        out_gt = torch.empty((n, 1, H, W), dtype=torch.int64, device=img.device)
    _lib.check(_L().gs_batch_rescale(img.data_ptr(), gt.data_ptr() if gt is not None else None,
                                     n, h, w, out.data_ptr(),
                                     out_gt.data_ptr() if gt is not None else None, H, W,
                                     current_stream_ptr()), "gs_batch_rescale")
    BATCH_RESCALE_CALLS += 1
    return out, out_gt
