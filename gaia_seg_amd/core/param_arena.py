"""Flat fp32 arenas for parameters, gradients and optimizer state -- SGD momentum, or AdamW's two moments and
per-parameter step counters (laid out for 288 GB of HBM3E).

Every parameter of the supernet becomes a view into ONE contiguous buffer (and its gradient a view
into a second one with identical offsets), in forward order.  This gives
  * a fused SGD step over a few merged ranges instead of ~300 small tensors (K18: torch.optim.SGD of
    configs/_dynamic_/models/pspnet_ar50to101v2_gsync.py:175 — momentum 0.9, weight decay 5e-4),
  * zero-copy gradient buckets for the data-parallel all-reduce (the reducer all-reduces slices of
    the flat gradient buffer; nothing is packed or unpacked),
  * one memset to clear the gradients of a step.
Only the parameters that take part in the sampled subnet are touched by a step: depth-skipped
blocks get no gradient and no update at all (DECIDE); inactive width
slices of used tensors have zero gradient but do receive weight decay / momentum, like the
reference (they belong to a tensor that has a gradient).
"""
import torch

from ..hip import lib as _lib
from ..hip.runtime import current_stream_ptr, round_up
from .bricks import hwio_logical_view

_ALIGN = 64  # floats: 256-byte aligned segments (float4 loads need 16 B; keep cache lines whole)


def arena_layout(model):
    """[(name, parameter, physical shape or None, offset, physical numel)], total elements: where every
    parameter sits in the flat arenas (forward order, 256-byte aligned segments).  Host arithmetic
    only — `bench.py --plan-only` sizes the gradient buckets from it without a GPU."""
    off, layout = 0, []
    for name, p in model.named_parameters():
        phys = getattr(p, "_gs_phys_shape", None)
        n_phys = 1
        for s in (phys if phys is not None else p.shape):
            n_phys *= s
        layout.append((name, p, phys, off, n_phys))
        off += round_up(max(n_phys, 1), _ALIGN)
    return layout, off


class ParamArena:
    def __init__(self, model):
        from .bricks import DynamicConv2d, relayout_conv_params
        for m in model.modules():  # (re)attach the physical-layout descriptors (lost by deepcopy)
            if isinstance(m, DynamicConv2d):
                relayout_conv_params(m)
        params = [(n, p) for n, p in model.named_parameters()]
        if not params:
            raise ValueError("model has no parameters")
        dev = params[0][1].device
        if dev.type != "cuda":
            raise _lib.HipLibraryError("ParamArena needs the model on the MI355X (got %s)" % dev)
        self.device = dev
        self.segments = {}   # id(param) -> (offset, numel_phys)
        self.names = {}
        layout, off = arena_layout(model)
        self.numel = off
        self.flat_param = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_mom = torch.zeros(off, dtype=torch.float32, device=dev)
        self._layout = [(name, p, phys, o, n) for name, p, phys, o, n in layout]
        for name, p, phys, o, n in layout:
            pv = self._view(self.flat_param, p, phys, o, n)
            pv.copy_(p.data)
            p.data = pv
            p.grad = self._view(self.flat_grad, p, phys, o, n)
            # gradients now always exist: drop the lazy factories
            if hasattr(p, "_gs_grad_factory"):
                del p._gs_grad_factory
            self.segments[id(p)] = (o, round_up(max(n, 1), _ALIGN))
            self.names[id(p)] = name
        self._range_cache = {}
        # True while every gradient element is zero outside a running step (see zero_grad)
        self.grads_clean = False
        # gradient accumulation buffer of the sandwich iterations (core/runner.py), allocated at
        # first use; zero outside a running iteration
        self.flat_acc = None
        # parameter groups (set_param_groups): None = the ungrouped gs_sgd_step path
        self.groups = None
        self.group_epoch = 0          # counts set_param_groups calls (part of the step-graph key)
        self.group_hyper = None       # device {momentum, grad_scale, n_groups, 0, lr_0, wd_0, ...}
        self._group_hyper_vals = None
        self._tables = None           # optimizer.ChunkTableCache of the current grouping
        # while a list: every device tensor a gs_sgd_step_groups launch names is appended (the runner
        # sets it around a graph capture and keeps the list with the graph)
        self.capture_refs = None
        # the optimizer kind (set_optimizer): 'SGD' keeps flat_mom alone; 'AdamW' adds the second
        # moment, one int32 step counter per parameter and an fp64 hyper table
        self.optimizer = "SGD"
        self.flat_var = None          # AdamW exp_avg_sq (flat_mom is its exp_avg)
        self.steps = None             # AdamW: int32 [number of parameters], torch's state['step']
        self.betas, self.eps = None, None
        self.adamw_hyper = None       # device doubles, GS_ADAMW_HYPER_DOUBLES (gaiaseg_hip.h)
        self._adamw_hyper_vals = None
        self._group_of_param, self._chunk_floats = None, None

    # ---- optimizer kind ----
    def set_optimizer(self, kind, betas=(0.9, 0.999), eps=1e-8):
        """'SGD' (the state the arena is built in) or 'AdamW': allocates ``flat_var`` and ``steps``
        (zero) and from here on the chunk tables are per parameter (every chunk carries its
        parameter's slot in ``steps``).  An SGD arena allocates nothing for AdamW."""
        if kind not in ("SGD", "AdamW"):
            raise NotImplementedError("optimizer %r: only SGD and AdamW" % (kind,))
        if kind == "AdamW":
            b1, b2 = (float(b) for b in betas)
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) > 0.0:
                raise ValueError("AdamW needs betas in [0, 1) and eps > 0, got %r, %r" % (betas, eps))
            self.betas, self.eps = (b1, b2), float(eps)
            if self.flat_var is None:
                self.flat_var = torch.zeros_like(self.flat_mom)
                self.steps = torch.zeros(len(self._layout), dtype=torch.int32, device=self.device)
        else:
            self.flat_var = self.steps = self.betas = self.eps = None
        changed, self.optimizer = kind != self.optimizer, kind
        self._adamw_hyper_vals = None
        if changed and self._group_of_param is not None:      # tables of the other mode are void
            self.set_param_groups(self._group_of_param, self.groups, self._chunk_floats)

    def reset_optimizer_state(self):
        """Momentum / first moment, second moment and step counters back to zero."""
        with torch.no_grad():
            self.flat_mom.zero_()
            if self.flat_var is not None:
                self.flat_var.zero_()
                self.steps.zero_()

    # ---- parameter groups (paramwise_cfg, core/optimizer.py) ----
    def set_param_groups(self, group_of_param, n_groups=1, chunk_floats=None):
        """``group_of_param``: {parameter name: group index} over the trainable parameters (None
        switches grouping off).  From here on sgd_step takes one lr / weight decay PER GROUP and makes
        ONE gs_sgd_step_groups launch over a chunk table, whatever the number of fragments.
        Calling it again starts a new grouping: ``group_epoch`` moves on, so step graphs captured
        under the earlier one are never replayed (runner._graph_key); they keep their own tables."""
        from . import optimizer as _opt
        self.group_epoch += 1
        self._group_hyper_vals = None
        self._tables = None
        self._adamw_hyper_vals = None
        self._group_of_param, self._chunk_floats = group_of_param, chunk_floats
        if group_of_param is None:
            self.groups = None
            return
        if not 1 <= n_groups <= _lib.SGD_MAX_GROUPS:
            raise ValueError("n_groups must be in [1, %d], got %d" % (_lib.SGD_MAX_GROUPS, n_groups))
        unknown = set(group_of_param) - {name for name, *_ in self._layout}
        if unknown:
            raise KeyError("set_param_groups: no such parameters %s" % sorted(unknown)[:3])
        if any(not 0 <= g < n_groups for g in group_of_param.values()):
            raise ValueError("set_param_groups: group index outside [0, %d)" % n_groups)
        self.groups = n_groups
        self._tables = _opt.ChunkTableCache(
            _opt.segment_groups(self._layout, group_of_param, _ALIGN, per_param=self.optimizer == "AdamW"),
            chunk_floats or _opt.CHUNK_FLOATS,
            upload=lambda tab: torch.from_numpy(tab).to(self.device), numel=self.numel,
            n_slots=len(self._layout))
        # a fresh table per grouping: a graph of an earlier grouping keeps (and reads) its own
        self.group_hyper = torch.zeros(4 + 2 * _lib.SGD_MAX_GROUPS, dtype=torch.float32, device=self.device)
        if self.optimizer == "AdamW":
            self.adamw_hyper = torch.zeros(_lib.ADAMW_HYPER_DOUBLES, dtype=torch.float64, device=self.device)

    def chunk_table(self, ranges):
        """(device table, chunks, fragments) of ``ranges`` under the current grouping, built once per
        set of ranges (a host walk and one upload: never inside a graph capture -- the runner
        prepares the tables of a subnet in refresh_active)."""
        capturing = torch.cuda.is_current_stream_capturing()
        try:
            return self._tables.get(ranges, build=not capturing)
        except KeyError:
            raise RuntimeError("the chunk table of these ranges was not prepared before the capture") from None

    def write_group_hyper(self, lrs, weight_decays, momentum, grad_scale):
        """{momentum, grad_scale, n_groups, 0, lr_0, wd_0, ...} -> the device table in stream order
        (one tiny launch; skipped while the table already holds exactly these values)."""
        vals = (tuple(float(x) for x in lrs), tuple(float(x) for x in weight_decays),
                float(momentum), float(grad_scale))
        if len(vals[0]) != self.groups or len(vals[1]) != self.groups:
            raise ValueError("%d parameter groups need %d learning rates and weight decays, got %d / %d"
                             % (self.groups, self.groups, len(vals[0]), len(vals[1])))
        if vals == self._group_hyper_vals:
            return
        g = _lib.SgdGroups()
        for i, (lr, wd) in enumerate(zip(vals[0], vals[1])):
            g.lr_wd[2 * i], g.lr_wd[2 * i + 1] = lr, wd
        _lib.check(_lib.load().gs_sgd_set_group_hyper(self.group_hyper.data_ptr(), vals[2], vals[3],
                                                      self.groups, g, current_stream_ptr()),
                   "gs_sgd_set_group_hyper")
        self._group_hyper_vals = vals

    def write_adamw_hyper(self, lrs, weight_decays, grad_scale):
        """{betas, eps, grad_scale, n_groups, per-group lr / wd} -> the fp64 device table in stream
        order (one tiny launch; skipped while the table already holds exactly these values).  The
        values stay Python doubles all the way into the kernel's arguments."""
        vals = (tuple(float(x) for x in lrs), tuple(float(x) for x in weight_decays), float(grad_scale))
        if len(vals[0]) != self.groups or len(vals[1]) != self.groups:
            raise ValueError("%d parameter groups need %d learning rates and weight decays, got %d / %d"
                             % (self.groups, self.groups, len(vals[0]), len(vals[1])))
        if vals == self._adamw_hyper_vals:
            return
        g = _lib.AdamwGroups()
        for i, (lr, wd) in enumerate(zip(vals[0], vals[1])):
            g.lr_wd[2 * i], g.lr_wd[2 * i + 1] = lr, wd
        _lib.check(_lib.load().gs_adamw_set_group_hyper(self.adamw_hyper.data_ptr(), self.betas[0],
                                                        self.betas[1], self.eps, vals[2], self.groups,
                                                        g, current_stream_ptr()),
                   "gs_adamw_set_group_hyper")
        self._adamw_hyper_vals = vals

    @staticmethod
    def _view(flat, p, phys, off, n):
        seg = flat[off:off + n]
        if phys is None:
            return seg.view(p.shape)
        if len(phys) == 4:   # conv weight, physical HWIO
            return hwio_logical_view(seg.view(*phys), p.shape[0])
        if len(phys) == 1:   # padded conv bias
            return seg[:p.shape[0]]
        raise ValueError("unknown physical layout %s" % (phys,))

    # ---- ranges ----
    def ranges_for(self, params, key=None):
        """Merged [begin, end) element ranges covering ``params`` (cached by ``key``)."""
        if key is not None and key in self._range_cache:
            return self._range_cache[key]
        segs = sorted(self.segments[id(p)] for p in params)
        merged = []
        for o, n in segs:
            if merged and merged[-1][1] == o:
                merged[-1][1] = o + n
            else:
                merged.append([o, o + n])
        merged = [tuple(r) for r in merged]
        if key is not None:
            self._range_cache[key] = merged
        return merged

    def zero_grad(self, ranges=None, trust_clean=False):
        """Clear gradients.  ``trust_clean`` (passed only by IterBasedRunner, which owns the
        invariant): a no-op while ``grads_clean`` holds -- the buffer starts at zero and every
        sgd_step(zero_grad=True) clears what the step wrote, so a training loop that always follows
        backward with such a step over the same ranges never needs the fill kernels.  Any other caller
        (a manual train_step + backward in a test, a tool, a val workflow) gets a real clear: the flag
        says nothing about gradients produced outside the runner."""
        if trust_clean and self.grads_clean:
            return
        if ranges is None:
            self.flat_grad.zero_()
        else:
            for a, b in ranges:
                self.flat_grad[a:b].zero_()

    def sgd_step(self, ranges, lr, momentum=0.9, weight_decay=5e-4, grad_scale=1.0, zero_grad=False,
                 hyper=None):
        """torch.optim.SGD(momentum, weight_decay, dampening=0, nesterov=False) on the ranges.
        ``hyper``: device tensor {lr, momentum, weight_decay, grad_scale} read by the kernel at run
        time instead of the by-value arguments (step graphs, core/runner.py).
        With parameter groups set, ``lr`` and ``weight_decay`` are sequences (one value per group) and
        the whole step is ONE gs_sgd_step_groups launch over the chunk table of ``ranges``; a non-None
        ``hyper`` then means the caller has written the group table itself (write_group_hyper, outside
        the captured graph)."""
        L = _lib.load()
        st = current_stream_ptr()
        pb, gb, mb = self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.flat_mom.data_ptr()
        if self.groups is not None:
            table, n_chunks, _ = self.chunk_table(ranges)
            if n_chunks == 0:
                return
            if hyper is None:
                self.write_group_hyper(lr, weight_decay, momentum, grad_scale)
            elif self._group_hyper_vals is None:
                raise RuntimeError("sgd_step(hyper=...) with parameter groups before write_group_hyper")
            if self.capture_refs is not None:
                self.capture_refs += [table, self.group_hyper]
            _lib.check(L.gs_sgd_step_groups(pb, gb, mb, table.data_ptr(), n_chunks,
                                            self.group_hyper.data_ptr(), 1 if zero_grad else 0, st),
                       "gs_sgd_step_groups")
            return
        if hyper is not None:
            hp = hyper.data_ptr()
            for a, b in ranges:
                _lib.check(L.gs_sgd_step_hyper(pb + 4 * a, gb + 4 * a, mb + 4 * a, b - a, hp,
                                               1 if zero_grad else 0, st), "gs_sgd_step_hyper")
            return
        for a, b in ranges:
            _lib.check(L.gs_sgd_step(pb + 4 * a, gb + 4 * a, mb + 4 * a, b - a, lr, momentum,
                                     weight_decay, grad_scale, 1 if zero_grad else 0, st),
                       "gs_sgd_step")

    def adamw_step(self, ranges, lr, weight_decay, grad_scale=1.0, zero_grad=False, hyper=None):
        """torch.optim.AdamW(betas, eps, amsgrad=False) on the ranges: ONE gs_adamw_step_groups call
        over the per-parameter chunk table of ``ranges`` (the step kernel, then the launch that
        advances the counters of the parameters it stepped).  ``lr`` / ``weight_decay``: one value
        per parameter group.  A non-None ``hyper`` means the caller has written the hyper table
        itself (write_adamw_hyper, outside a captured graph)."""
        if self.optimizer != "AdamW":
            raise RuntimeError("adamw_step on an arena in %s mode (set_optimizer('AdamW', ...))" % self.optimizer)
        if self.groups is None:
            raise RuntimeError("adamw_step needs parameter groups (set_param_groups; one group is fine)")
        table, n_chunks, _ = self.chunk_table(ranges)
        if n_chunks == 0:
            return
        if hyper is None:
            self.write_adamw_hyper(lr, weight_decay, grad_scale)
        elif self._adamw_hyper_vals is None:
            raise RuntimeError("adamw_step(hyper=...) before write_adamw_hyper")
        if self.capture_refs is not None:
            self.capture_refs += [table, self.adamw_hyper]
        _lib.check(_lib.load().gs_adamw_step_groups(
            self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.flat_mom.data_ptr(),
            self.flat_var.data_ptr(), self.steps.data_ptr(), self.steps.numel(), table.data_ptr(),
            n_chunks, self.adamw_hyper.data_ptr(), 1 if zero_grad else 0, current_stream_ptr()),
            "gs_adamw_step_groups")

    def accumulate(self, ranges, into="buffer"):
        """Move gradients between the gradient arena and the accumulation buffer over ``ranges``
        (one gs_grad_accumulate launch per merged range):
          into="buffer": flat_acc += flat_grad; flat_grad = 0  (after each member's backward: the
                         weight-gradient kernels overwrite their gradient, they cannot add to it)
          into="grad":   flat_grad += flat_acc; flat_acc = 0  (before the iteration's one SGD step)
        Both sides are zero over ``ranges`` afterwards except the destination."""
        if into not in ("buffer", "grad"):
            raise ValueError("into must be 'buffer' or 'grad', got %r" % (into,))
        if self.flat_acc is None:
            self.flat_acc = torch.zeros_like(self.flat_grad)
        L = _lib.load()
        st = current_stream_ptr()
        dst, src = (self.flat_acc, self.flat_grad) if into == "buffer" else (self.flat_grad, self.flat_acc)
        db, sb = dst.data_ptr(), src.data_ptr()
        for a, b in ranges:
            _lib.check(L.gs_grad_accumulate(db + 4 * a, sb + 4 * a, b - a, st), "gs_grad_accumulate")

    def momentum_views(self):
        """{parameter name: momentum buffer as a LOGICAL (OIHW / plain) view of the flat arena}."""
        return {name: self._view(self.flat_mom, p, phys, o, n) for name, p, phys, o, n in self._layout}

    def variance_views(self):
        """{parameter name: exp_avg_sq as a LOGICAL view of the flat arena} (AdamW mode)."""
        return {name: self._view(self.flat_var, p, phys, o, n) for name, p, phys, o, n in self._layout}

    SGD_FORMAT, ADAMW_FORMAT = "gaia_seg_amd.sgd_momentum.v1", "gaia_seg_amd.adamw.v1"

    def state_dict(self):
        """Optimizer state keyed by parameter name in the logical layout (contiguous OIHW for conv
        weights), so that neither the arena offsets nor the physical HWIO layout leak into a
        checkpoint (tools/train_supernet.py:197-202 stores `optimizer` next to `state_dict`).
        AdamW mode: per name {step, exp_avg, exp_avg_sq}, with the betas and eps alongside."""
        if self.optimizer == "AdamW":
            steps = self.steps.cpu().tolist()
            mom, var = self.momentum_views(), self.variance_views()
            return {"format": self.ADAMW_FORMAT, "betas": tuple(self.betas), "eps": self.eps,
                    "state": {name: {"step": int(steps[i]),
                                     "exp_avg": mom[name].detach().clone().contiguous(),
                                     "exp_avg_sq": var[name].detach().clone().contiguous()}
                              for i, (name, *_r) in enumerate(self._layout)}}
        return {"format": self.SGD_FORMAT,
                "state": {k: v.detach().clone().contiguous() for k, v in self.momentum_views().items()}}

    def _load_adamw_state(self, sd, warn):
        state = sd.get("state") if isinstance(sd, dict) else None
        if not isinstance(sd, dict) or sd.get("format") != self.ADAMW_FORMAT or not isinstance(state, dict):
            warn("optimizer state of a foreign format (not %s): AdamW moments and step counters "
                 "restart from zero" % self.ADAMW_FORMAT)
            self.reset_optimizer_state()
            return False
        self.reset_optimizer_state()
        mom, var = self.momentum_views(), self.variance_views()
        steps = self.steps.cpu()
        missing = [k for k in mom if k not in state]
        with torch.no_grad():
            for i, (name, *_r) in enumerate(self._layout):
                ent = state.get(name)
                if ent is None:
                    continue
                for key, views in (("exp_avg", mom), ("exp_avg_sq", var)):
                    if tuple(views[name].shape) != tuple(ent[key].shape):
                        raise RuntimeError("%s of %s: checkpoint %s vs model %s"
                                           % (key, name, tuple(ent[key].shape), tuple(views[name].shape)))
                    views[name].copy_(ent[key])
                steps[i] = int(ent["step"])
            self.steps.copy_(steps)
        if missing:
            warn("optimizer state lacks %d parameters (e.g. %s): their AdamW state is zero"
                 % (len(missing), missing[0]))
        return True

    def load_state_dict(self, sd, logger=None):
        """Accepts this build's format; any other optimizer state (e.g. a torch.optim.SGD state_dict
        of an mmcv checkpoint, whose integer keys carry no parameter names) is skipped with a warning
        and the momentum restarts from zero."""
        import warnings
        if self.optimizer == "AdamW":
            return self._load_adamw_state(sd, logger.warning if logger is not None else warnings.warn)
        state = sd.get("state") if isinstance(sd, dict) else None
        if not isinstance(sd, dict) or sd.get("format") != "gaia_seg_amd.sgd_momentum.v1" \
                or not isinstance(state, dict):
            msg = "optimizer state of a foreign format: momentum buffers restart from zero"
            (logger.warning if logger is not None else warnings.warn)(msg)
            return False
        views = self.momentum_views()
        missing = [k for k in views if k not in state]
        with torch.no_grad():
            for k, v in state.items():
                if k in views:
                    if tuple(views[k].shape) != tuple(v.shape):
                        raise RuntimeError("momentum of %s: checkpoint %s vs model %s"
                                           % (k, tuple(v.shape), tuple(views[k].shape)))
                    views[k].copy_(v)
        if missing:
            msg = "optimizer state lacks %d parameters (e.g. %s): their momentum is zero" % (
                len(missing), missing[0])
            (logger.warning if logger is not None else warnings.warn)(msg)
        return True
