"""Stream state of the MI355X path: which HIP stream a kernel is launched on, and its scratch.

What lives here: the raw handle of torch's current stream (``current_stream_ptr``), the grow-only
scratch buffer per stream slot (``WORKSPACE``), the weight-gradient side stream with its batched job
queue (``queue_wgrad`` / ``flush_wgrads`` / ``join_side_streams`` / ``deferred_join`` /
``side_checkpoint``), the branch streams (``Branch``, ``branch_scope``, ``prefork_branch``,
``join_branch``) and the scope an autograd node's backward runs in (``adopt_current_stream``).
It needs only ``lib`` and torch; ``runtime`` (activations, the tape) and ``ops`` (the operator
catalogue, with the policy flags that say WHEN a branch or the side stream is used) build on it.
"""
import ctypes
import os

import torch

from . import lib as _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_ptr():
    """hipStream_t of torch's current stream on the current device (raw handle: this is called
    once per kernel launch, torch.cuda.current_stream() costs ~9 us of host time each)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class _Workspace:
    """Grow-only scratch buffer per device and stream slot (split-K slabs, reduction partials).

    All kernels of one in-order queue share a buffer.  ``slot`` selects the queue: 0 = the training
    stream, 1 / 2 = the branch streams (projection shortcuts, the auxiliary head); whoever switches
    the current stream switches the slot with it."""

    def __init__(self):
        self._buf = {}
        self._retired = []   # outgrown buffers: captured step graphs may still point into them
        self.slot = 0

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 256)
        key = (device.type, device.index, self.slot)
        buf = self._buf.get(key)
        if buf is None or buf.numel() < nbytes:
            # round up generously so later, larger requests rarely reallocate
            size = max(nbytes, 1 << 20)
            size = 1 << (size - 1).bit_length()
            if buf is not None:
                self._retired.append(buf)
            buf = torch.empty(size, dtype=torch.uint8, device=device)
            self._buf[key] = buf
        return buf

    def reserve(self, nbytes, device):
        self.get(nbytes, device)


WORKSPACE = _ws = _Workspace()


def _notify(param):
    """Tell the gradient reducer (core/dist.py), if one listens, that ``param.grad`` is queued."""
    hook = param.__dict__.get("_gs_grad_ready")
    if hook is not None:
        hook(param)


# ---- stream state ------------------------------------------------------------------------------
# Besides the training stream a device has one weight-gradient side stream and up to two branch
# streams.  Every order between them is set by ``_fork`` (one event recorded on one stream, waited
# for on another); the dirty flags say which of them hold work that the training stream has not
# joined yet.  (More weight-gradient streams, an optimizer stream inside backward, stream priorities
# and an earlier fork of the auxiliary head were measured and removed: profiles/r04_stream_experiments.md.)
class _DeviceStreams:
    __slots__ = ("side", "side_dirty", "branch", "origin", "branch_dirty")

    def __init__(self):
        self.side = None           # the weight-gradient stream (created on first use)
        self.side_dirty = False
        self.branch = {}           # slot -> branch stream (created on first use)
        self.origin = {}           # slot -> raw handle of the stream the branch was last forked from
        self.branch_dirty = set()  # slots with work the origin has not joined yet


_streams = {}   # (device type, index) -> _DeviceStreams


def _state(dev):
    st = _streams.get((dev.type, dev.index))
    if st is None:
        st = _streams[(dev.type, dev.index)] = _DeviceStreams()
    return st


def _fork(src, dst, dev):
    """Stream ``dst`` waits for everything queued on stream ``src`` so far (raw handles)."""
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gs_stream_fork(src, dst), "gs_stream_fork")


# ---- weight gradients on a side stream -------------------------------------------------------
# In backward the weight gradient of a conv is needed only by the optimizer (and the gradient
# all-reduce), while the data gradient is on the critical path.  The wgrad kernels (MFMA-bound) are
# therefore launched on a second HIP stream, fenced by events, and run concurrently with the
# BN-backward / dgrad kernels of the following layers (HBM-bound) on the main stream.  The main
# stream joins the side stream at the end of every tape backward and before a gradient bucket is
# handed to RCCL.  (Whether the convs use it at all is ops.SIDE_WGRAD.)
_ws_side = _Workspace()


def _side_stream(dev):
    st = _state(dev)
    if st.side is None:
        st.side = torch.cuda.Stream(device=dev)
    return st.side


def side_stream(dev):
    """The weight-gradient stream of ``dev``, or None while nothing has used it."""
    st = _streams.get((dev.type, dev.index))
    return st.side if st is not None else None


# Weight gradients are handed to the side stream in BATCHES: every hand-over costs one event on the
# main stream (hipEventRecord puts a marker packet into the queue; the r02 kernel trace shows a
# ~7 us bubble behind each of them, 57 per R50 step).  A conv's backward therefore only queues its
# weight-gradient job; after WGRAD_BATCH jobs (or at the end of a tape, or before a gradient bucket
# is all-reduced) one event covers them all and the jobs are launched on the side stream.  The
# "gradient ready" notifications of the reducer fire when the job is actually enqueued.
WGRAD_BATCH = max(1, int(os.environ.get("GS_WGRAD_BATCH", "4")))
_wgrad_jobs = []
_wgrad_stream = None   # raw handle of the stream the queued jobs' operands were produced on


_side_keep = []   # (dy, x) of weight-gradient kernels launched on the side stream, until the join


def queue_wgrad(d, x, dy, weight, gw, need, dev):
    """x: Act (kept alive until the launch), dy: gradient of the conv output, gw: weight.grad."""
    global _wgrad_stream
    st = current_stream_ptr()
    if _wgrad_jobs and st != _wgrad_stream:
        flush_wgrads()     # one event covers one batch: a batch never mixes producer streams
    _wgrad_stream = st
    _wgrad_jobs.append((d, x, dy, weight, gw, need, dev))
    if len(_wgrad_jobs) >= WGRAD_BATCH:
        flush_wgrads()


def flush_wgrads():
    """One event for all queued weight-gradient jobs, then launch them on the side stream."""
    global _wgrad_jobs
    if not _wgrad_jobs:
        return
    jobs, _wgrad_jobs = _wgrad_jobs, []
    L = _lib.load()
    dev = jobs[0][6]
    side = _side_stream(dev)
    _fork(_wgrad_stream, side.cuda_stream, dev)
    with torch.cuda.device(dev):
        for d, x, dy, weight, gw, need, _ in jobs:
            ws_s = _side_workspace(need, dev, side)
            # dy and x must outlive the side-stream kernel that reads them: they are kept referenced
            # until the main stream has joined the side stream (join_side_streams) instead of being
            # handed to the caching allocator with record_stream (two calls and one pending event
            # per convolution and step)
            _side_keep.append((dy, x))
            # (descriptors are shared per layer: the operand-loader coefficients are per call)
            d.in_affine = x.affine.data_ptr() if x.affine is not None else None
            _lib.check(L.gs_conv2d_wgrad(ctypes.byref(d), x.ptr, dy.data_ptr(), gw.data_ptr(),
                                         ws_s.data_ptr(), ws_s.numel(), side.cuda_stream),
                       "gs_conv2d_wgrad")
    _state(dev).side_dirty = True
    for job in jobs:
        _notify(job[3])


_deferred = None   # the deferred_join scope a backward runs in (None: every tape joins the side stream)


class deferred_join:
    """``with streams.deferred_join() as dj: loss.backward()`` -- the tapes hand their weight gradients
    to the side stream but do not join it (``end_tape_backward``): the caller overlaps the optimizer
    step with the last weight gradients and joins afterwards (join_side_streams).  ``dj.checkpoint``:
    the events ``side_checkpoint`` left on the side streams (every weight gradient queued before them
    is done once they have fired), or None when backward crossed no checkpoint.  Nothing outside
    this scope switches the protocol on or off."""

    def __init__(self):
        self.checkpoint = None

    def __enter__(self):
        global _deferred
        _deferred = self
        return self

    def __exit__(self, *exc):
        global _deferred
        _deferred = None
        return False


def end_tape_backward():
    """End of a tape's backward replay (runtime.Tape.backward): the queued weight gradients go to the
    side stream, and the current stream joins it unless a ``deferred_join`` scope does that later
    (runner: after the early part of the optimizer step)."""
    if _deferred is not None:
        flush_wgrads()
    else:
        join_side_streams()


def side_checkpoint(tape):
    """Mark a point of the backward replay (recorded in forward order, so it fires when backward
    crosses it): all weight gradients of the layers AFTER this point have been handed to the side
    stream; an event on the side stream lets the optimizer update those parameters while the side
    stream still works on the layers before the point (the runner waits on deferred_join.checkpoint)."""
    def backward():
        dj = _deferred
        if dj is None:
            return
        flush_wgrads()
        events = [st.side.record_event() for st in _streams.values() if st.side_dirty]
        dj.checkpoint = events or None
    tape.record(backward)


def join_side_streams(dev=None):
    """Make the current stream wait for the weight-gradient kernels queued on the side stream."""
    flush_wgrads()
    for key, st in _streams.items():
        if st.side_dirty and (dev is None or (dev.type, dev.index) == key):
            _fork(st.side.cuda_stream, current_stream_ptr(), st.side.device)
            st.side_dirty = False
    if dev is None or not any(st.side_dirty for st in _streams.values()):
        # everything the side stream read is now ordered before whatever the current stream does
        # next: the operands may go back to the allocator
        _side_keep.clear()


def side_stream_after_main(dev):
    """The side stream, made to wait for everything queued so far on the current stream and on the
    branch streams of this device (a gradient bucket holds BatchNorm gradients written on the
    training stream and, where a branch ran, on the branch stream)."""
    s = _side_stream(dev)
    st = _state(dev)
    cur = current_stream_ptr()
    _fork(cur, s.cuda_stream, dev)
    others = set()
    for slot, br in st.branch.items():
        if slot in st.branch_dirty:
            others.add(br.cuda_stream)
            others.add(st.origin[slot])
    for other in others:
        if other != cur:
            _fork(other, s.cuda_stream, dev)
    st.side_dirty = True   # the main stream joins it at the end of backward
    return s


def _side_workspace(need, dev, side):
    """Split-K scratch of the side stream (allocated under that stream, so the caching allocator
    orders its reuse against that stream's kernels)."""
    buf = _ws_side._buf.get((dev.type, dev.index, 0))
    if buf is not None and buf.numel() >= need:
        return buf
    with torch.cuda.stream(side):
        return _ws_side.get(need, dev)


def reserve_workspaces(dev, nbytes=192 << 20):
    """Size the main and the side-stream scratch buffers for the largest request a convolution of
    the supernet can make (96 MiB of split-K slabs + reduction partials), so that a step graph
    capture never sees a workspace being (re)allocated."""
    _ws.get(nbytes, dev)
    _side_workspace(nbytes, dev, _side_stream(dev))


# ---- the branch stream -------------------------------------------------------------------------
# A bs-2 step is ~450 launches of 5-100 us, each a single round of 1-4 workgroups per CU with its
# ramp and its tail; the only thing that fills those is ANOTHER launch running beside
# it.  Two sub-chains of the network are independent of the main chain and run on a second in-order
# queue, fenced by events:
#   * the projection shortcut (conv + BN) of a stage's first block, beside conv1 -> conv2, forward
#     and backward (gaiaseg/models/utils/dynamic_res_layer.py:70-125);
#   * the auxiliary head with its loss, beside the decode head
#     ("dynamic_encoder_decoder-distill-backup (1).py":85-143: two independent consumers of x).
# Same kernels, same operands, same results; only the queue differs.  GS_BRANCH=0 keeps one queue;
# the two uses are switched separately by ops.BRANCH_SHORTCUT / ops.BRANCH_AUX.
BRANCH = os.environ.get("GS_BRANCH", "1") != "0"
SLOT_SHORTCUT, SLOT_AUX = 1, 2   # scratch slot / branch stream index (0 = the training stream)
_branch_slot_of = {}     # raw stream handle -> slot (adopt_current_stream)
_branch_cb_armed = False


def _branch_stream(dev, slot):
    st = _state(dev)
    s = st.branch.get(slot)
    if s is None:
        s = st.branch[slot] = torch.cuda.Stream(device=dev)
        _branch_slot_of[s.cuda_stream] = slot
    return s


def on_branch():
    return _ws.slot != 0


def prefork_branch(dev, slot):
    """Make branch stream ``slot`` wait for what is queued on the current stream NOW; a later
    ``branch_scope(..., forked=True)`` then starts from this point of the current stream instead of
    from its tail at that time (the auxiliary head forks behind the backbone while the host goes on
    to queue the decode head)."""
    if not BRANCH or dev.type != "cuda" or on_branch():
        return
    br = _branch_stream(dev, slot)
    st = _state(dev)
    cur = current_stream_ptr()
    _fork(cur, br.cuda_stream, dev)
    st.origin[slot] = cur
    st.branch_dirty.add(slot)


def _enter_branch(dev, slot, fork=True):
    """Fork: branch stream ``slot`` waits for everything queued on the current stream, then becomes
    the current stream (with its own scratch buffers).  Returns the stream to go back to."""
    flush_wgrads()            # (backward) queued weight gradients belong to the stream we leave
    br = _branch_stream(dev, slot)
    st = _state(dev)
    prev = torch.cuda.current_stream(dev)
    if fork or st.origin.get(slot) != prev.cuda_stream:
        _fork(prev.cuda_stream, br.cuda_stream, dev)
        st.origin[slot] = prev.cuda_stream
    st.branch_dirty.add(slot)
    torch.cuda.set_stream(br)
    _ws.slot = slot
    return prev


def _leave_branch(prev):
    flush_wgrads()
    torch.cuda.set_stream(prev)
    _ws.slot = 0


def join_branch(dev, slot):
    """The current stream waits for everything queued on branch stream ``slot`` so far."""
    st = _state(dev)
    if slot in st.branch_dirty:
        _fork(st.branch[slot].cuda_stream, current_stream_ptr(), dev)


def join_branch_streams():
    """End of a step's backward: the stream the branches were forked from waits for them."""
    global _branch_cb_armed
    _branch_cb_armed = False
    for st in _streams.values():
        for slot, br in st.branch.items():
            if slot in st.branch_dirty:
                _fork(br.cuda_stream, st.origin[slot], br.device)
        st.branch_dirty.clear()


class adopt_current_stream:
    """``with streams.adopt_current_stream():`` around the body of an autograd node's backward.
    Autograd has made the node's forward stream current (a head or a loss evaluated under
    ``branch_scope`` comes back with the branch stream current): the scope picks the matching
    scratch slot and puts the previous one back on exit, exceptions included; queued weight
    gradients are flushed where the slot changes (they belong to the stream being left).  On a branch
    stream it also arranges for the final join (nothing else would order a later reader on the
    training stream behind, e.g., the auxiliary head's BatchNorm gradients when no upstream node
    consumes a gradient of this one)."""

    __slots__ = ("_prev",)

    def __enter__(self):
        global _branch_cb_armed
        self._prev = prev = _ws.slot
        if _branch_slot_of:
            slot = _branch_slot_of.get(current_stream_ptr(), 0)
            if slot != prev:
                flush_wgrads()
            _ws.slot = slot
            if slot and not _branch_cb_armed:
                _branch_cb_armed = True
                torch.autograd.Variable._execution_engine.queue_callback(join_branch_streams)
        return self

    def __exit__(self, *exc):
        if _ws.slot != self._prev:
            flush_wgrads()
            _ws.slot = self._prev
        return False


class branch_scope:
    """``with streams.branch_scope(dev):`` evaluate a whole sub-model (the auxiliary head and its
    loss) on a branch stream.  Its autograd nodes run their backward there too (autograd's stream
    semantics); ``streams.join_branch(dev, slot)`` afterwards orders the current stream behind it.
    ``forked``: the branch already waits for the right point of the current stream
    (``prefork_branch``)."""

    def __init__(self, dev, enabled=True, slot=SLOT_AUX, forked=False):
        self.dev, self.slot, self.forked = dev, slot, forked
        self.on = bool(enabled and BRANCH and dev.type == "cuda" and not on_branch())
        self.prev = None

    def __enter__(self):
        if self.on:
            self.prev = _enter_branch(self.dev, self.slot, fork=not self.forked)
        return self

    def __exit__(self, *exc):
        if self.on:
            _leave_branch(self.prev)
        return False


class Branch:
    """A sub-chain of ONE tape evaluated on a branch stream.

        br = Branch(tape, dev)
        with br:                          # forward: fork; ops run (and record) on the branch
            identity = shortcut(x)
        a = conv1(x)
        br.record_backward_join(tape)     # backward: everything recorded BEFORE this point runs
                                          #           after the branch's backward has finished
        b = conv2(a)
        br.record_backward_body(tape)     # backward: fork here, replay the branch's closures
        br.join()                         # forward: the current stream waits for the branch
        out = conv3(b) + identity

    Backward order on the host: conv3, [fork, branch body], conv2, [join], conv1 — the branch's data
    gradient is the FIRST writer of x.g, conv1's accumulates onto it after the join.  With the
    branch switched off the same closures run in the same order on one stream."""

    __slots__ = ("tape", "dev", "on", "ops", "slot", "_saved", "_prev")

    def __init__(self, tape, dev, enabled=True, slot=SLOT_SHORTCUT):
        self.tape, self.dev, self.slot = tape, dev, slot
        self.on = bool(enabled and BRANCH and dev.type == "cuda" and not on_branch())
        self.ops = []
        self._saved = self._prev = None

    def __enter__(self):
        self._saved = self.tape.ops
        self.tape.ops = self.ops
        if self.on:
            self._prev = _enter_branch(self.dev, self.slot)
        return self

    def __exit__(self, *exc):
        if self.on:
            _leave_branch(self._prev)
        self.tape.ops = self._saved
        self._saved = self._prev = None
        return False

    def join(self):
        if self.on:
            join_branch(self.dev, self.slot)

    def record_backward_join(self, tape):
        if not self.on:
            return
        dev, slot = self.dev, self.slot
        tape.record(lambda: join_branch(dev, slot))

    def record_backward_body(self, tape):
        body, dev, on, slot = self.ops, self.dev, self.on, self.slot

        def backward():
            prev = _enter_branch(dev, slot) if on else None
            try:
                for fn in reversed(body):
                    fn()
            finally:
                if on:
                    _leave_branch(prev)
        if body:
            tape.record(backward)
