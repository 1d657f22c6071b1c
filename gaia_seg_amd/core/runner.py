"""Iteration-based training loop with hook points (mmcv IterBasedRunner contract) and the hooks
the supernet trainer registers (gaiaseg/apis/train.py:115-186):

  PolyLrUpdaterHook   lr_config = dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False)
                      (configs/_dynamic_/models/pspnet_ar50to101v2_gsync.py:177)
  ArenaOptimizerHook  zero_grad -> loss.backward() -> (RCCL bucket all-reduce) -> fused SGD step
  ManipulateArchHook  gaivision hook (gaiaseg/apis/train.py:142-146): before every train iteration
                      sample a meta, make it identical on all ranks, manipulate_arch
  SandwichHook        in-place distillation (tools/train_supernet.py:180-187, US-Nets sandwich rule):
                      every iteration trains [MAX, MIN, random x N] with one SGD step
  TextLoggerHook / CheckpointHook
"""
import os
import time
from collections import OrderedDict

import torch

from . import dist as gdist
from .dynamic import fold_dict
from .input_shape import INPUT_SHAPE_KEY, rescale_batch
from .model_space import arch_key, parse_input_shape


class Hook:
    in_graph = False   # True: after_train_iter only enqueues device work and may be graph-captured

    def before_run(self, runner):
        pass

    def after_run(self, runner):
        pass

    def before_train_iter(self, runner):
        pass

    def after_train_iter(self, runner):
        pass

    def every_n_iters(self, runner, n):
        return (runner.iter + 1) % n == 0 if n > 0 else False


class ManipulateArchHook(Hook):
    """One subnet per iteration: rank 0 draws a meta from the train sampler, the draw is broadcast
    (every rank must run the same subnet: the gradient buckets assume it), then
    ``model.manipulate_arch(fold_dict(meta)['arch'])`` (DECIDE)."""

    def __init__(self, sampler):
        self.sampler = sampler
        self.history = []

    def before_train_iter(self, runner):
        meta = self.sampler.sample() if gdist.rank() == 0 else None
        meta = gdist.broadcast_object(meta, src=0)
        runner.set_arch(meta)
        self.history.append(meta.get("name", "random"))


def full_arch_meta(model):
    """The supernet's largest architecture in fold_dict form ({'backbone': {'stem': .., 'body': ..}})."""
    bb = model.backbone
    own = getattr(bb, "full_arch_meta", None)   # a backbone with another search space states its own
    if own is not None:
        return {"backbone": own()}
    stem = bb.stem_width
    return {"backbone": {"stem": {"width": list(stem) if isinstance(stem, (list, tuple)) else stem},
                         "body": {"width": list(bb.body_width), "depth": list(bb.body_depth)}}}


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def check_sandwich_model(model):
    """In-place distillation needs heads whose teacher kwargs line up with what the MAX member hands
    out (the decode head's logits as 'teacher_logits', the auxiliary head's as 'aux_teacher_logits'):
    a PSP decode head and at most one FCN auxiliary head.  Anything else is refused here rather than
    guessed: an FCN decode head would read the auxiliary teacher's logits (another resolution), a
    UPer head has no distillation branch (its reference forward_train takes no kwargs).  A fixed
    teacher (DynamicDistiller) does not combine with the sandwich: its forward_train takes no teacher
    logits."""
    if getattr(model, "fixed_teacher", False):
        raise ValueError("use_distillation (sandwich) with a %s is not supported: the segmentor "
                         "distils from its own fixed teacher" % type(model).__name__)
    dec = model.decode_head
    if isinstance(dec, torch.nn.ModuleList):
        raise ValueError("use_distillation: a cascade of decode heads (%s) is not supported: the MAX member "
                         "hands out one 'teacher_logits' map, a cascade has one per stage"
                         % type(model).__name__)
    if getattr(dec, "kd_teacher_key", None) != "teacher_logits":
        raise ValueError(
            "use_distillation: the decode head must be a DynamicPSPHead (it reads 'teacher_logits'); "
            "%s %s" % (type(dec).__name__,
                       "reads the auxiliary teacher's logits 'aux_teacher_logits'"
                       if getattr(dec, "kd_teacher_key", None) else "has no distillation branch"))
    aux = getattr(model, "auxiliary_head", None)
    if aux is None:
        return
    if isinstance(aux, torch.nn.ModuleList):
        raise ValueError("use_distillation: a list of auxiliary heads has no teacher mapping "
                         "(the reference hands out one 'aux_logits')")
    if getattr(aux, "kd_teacher_key", None) != "aux_teacher_logits":
        raise ValueError("use_distillation: the auxiliary head must be a DynamicFCNHead (it reads "
                         "'aux_teacher_logits'); %s has no distillation branch" % type(aux).__name__)


SANDWICH_INPUT_SHAPE = ("apply_input_shape with use_distillation (sandwich) is not supported: teacher "
                        "and students at different resolutions are out of scope")


class SandwichHook(Hook):
    """In-place distillation (tools/train_supernet.py:180-187; US-Nets' sandwich rule): before every
    train iteration rank 0 draws the member list with ``ConcatSampler.candidates()`` -- MAX, MIN, then
    the random draws -- and broadcasts it; the runner then trains every member on the same batch, the
    students against the MAX member's detached logits, and takes ONE SGD step on the sum of their
    gradients (IterBasedRunner._sandwich_iter).  ``kd_cfg``: T, distillation_weight, interpolation
    (config key ``distill_cfg``; the reference's defaults 2, 0.5, False)."""

    def __init__(self, sampler, kd_cfg=None):
        from ..models.losses.distill_loss import KD_DEFAULTS
        if not hasattr(sampler, "candidates"):
            raise TypeError("SandwichHook needs a concat sampler (candidates()), got %s"
                            % type(sampler).__name__)
        unknown = set(kd_cfg or {}) - set(KD_DEFAULTS)
        if unknown:
            raise KeyError("distill_cfg: unknown keys %s (have %s)" % (sorted(unknown), sorted(KD_DEFAULTS)))
        self.sampler = sampler
        self.kd_cfg = dict(KD_DEFAULTS, **(kd_cfg or {}))
        self.history = []

    def before_run(self, runner):
        check_sandwich_model(runner.model)
        if runner.apply_input_shape:
            raise ValueError(SANDWICH_INPUT_SHAPE)

    def before_train_iter(self, runner):
        members = self.sampler.candidates() if gdist.rank() == 0 else None
        members = gdist.broadcast_object(members, src=0)
        if not members or _plain(fold_dict(members[0]).get("arch")) != full_arch_meta(runner.model):
            raise AssertionError("sandwich: the first member must be the supernet's full arch %s, got %s"
                                 % (full_arch_meta(runner.model), members[0] if members else None))
        runner.sandwich = (members, self.kd_cfg)
        self.history.append([m.get("name", "random") for m in members])


class LrUpdaterHook(Hook):
    """mmcv's LrUpdaterHook for iteration-based runs: before every iteration ``runner.lr`` becomes the
    policy's regular lr, warmed up while ``iter < warmup_iters`` (``warmup`` = 'constant': lr * ratio;
    'linear': lr * (1 - (1 - iter / warmup_iters) * (1 - ratio)); 'exp': lr * ratio ** (1 - iter /
    warmup_iters); mmcv's defaults None / 0 / 0.1).  On a runner with parameter groups every group is
    scheduled from ITS OWN initial lr (``runner.group_base_lr`` -> ``runner.group_lr``), as mmcv
    does, and ``runner.lr`` is group 0's.  Epoch-based warm-up and unknown keys are refused."""

    def __init__(self, by_epoch=False, warmup=None, warmup_iters=0, warmup_ratio=0.1,
                 warmup_by_epoch=False, **unknown):
        if unknown:
            raise KeyError("lr_config: unknown keys %s" % sorted(unknown))
        if warmup_by_epoch:
            raise NotImplementedError("lr_config.warmup_by_epoch=True: only warm-up by iteration")
        if warmup is not None:
            if warmup not in ("constant", "linear", "exp"):
                raise ValueError("lr_config.warmup=%r: must be 'constant', 'linear' or 'exp'" % (warmup,))
            if not warmup_iters > 0:
                raise ValueError("lr_config.warmup_iters must be positive with a warm-up, got %r"
                                 % (warmup_iters,))
            if not 0 < warmup_ratio <= 1.0:
                raise ValueError("lr_config.warmup_ratio must be in (0, 1], got %r" % (warmup_ratio,))
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, warmup_iters, warmup_ratio
        self.base_lr = None

    def before_run(self, runner):
        self.base_lr = runner.base_lr

    def regular_lr(self, runner, base_lr):
        return base_lr

    def warmup_lr(self, cur_iter, lr):
        if self.warmup is None or cur_iter >= self.warmup_iters:
            return lr
        if self.warmup == "constant":
            return lr * self.warmup_ratio
        if self.warmup == "linear":
            return lr * (1 - (1 - cur_iter / self.warmup_iters) * (1 - self.warmup_ratio))
        return lr * self.warmup_ratio ** (1 - cur_iter / self.warmup_iters)

    def get_lr(self, runner):
        return self.regular_lr(runner, self.base_lr)

    def before_train_iter(self, runner):
        runner.lr = self.warmup_lr(runner.iter, self.get_lr(runner))
        bases = getattr(runner, "group_base_lr", None)
        if bases is not None:
            runner.group_lr = [self.warmup_lr(runner.iter, self.regular_lr(runner, b)) for b in bases]
            runner.lr = runner.group_lr[0]


class PolyLrUpdaterHook(LrUpdaterHook):
    def __init__(self, power=1.0, min_lr=0.0, **kwargs):
        super().__init__(**kwargs)
        self.power, self.min_lr = power, min_lr

    def regular_lr(self, runner, base_lr):
        coeff = (1 - runner.iter / runner.max_iters) ** self.power
        return (base_lr - self.min_lr) * coeff + self.min_lr


class FixedLrUpdaterHook(LrUpdaterHook):
    # (reads runner.base_lr at every iteration and needs no before_run: tools and tests register this
    # hook and call train_iter without call_hook("before_run"), which has always worked)
    def before_run(self, runner):
        pass

    def get_lr(self, runner):
        return runner.base_lr


def _ranges_subtract(a, b):
    """a minus b for sorted lists of disjoint [begin, end) ranges."""
    out, j = [], 0
    for lo, hi in a:
        cur = lo
        while j < len(b) and b[j][1] <= cur:
            j += 1
        k = j
        while k < len(b) and b[k][0] < hi:
            if b[k][0] > cur:
                out.append((cur, b[k][0]))
            cur = max(cur, b[k][1])
            k += 1
        if cur < hi:
            out.append((cur, hi))
    return out


def _ranges_intersect(a, b):
    return _ranges_subtract(a, _ranges_subtract(a, b))


def _ranges_union(a, b):
    out = []
    for lo, hi in sorted(list(a) + list(b)):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(r) for r in out]


class ArenaOptimizerHook(Hook):
    """OptimizerHook for the flat-arena SGD: the step touches only the active subnet's ranges.

    Two instalments, each as early as its gradients are final:
      * everything but the stem and stage 1 once the weight-gradient stream has passed the
        checkpoint behind stage 1 (streams.side_checkpoint);
      * the stem and stage 1 after the weight-gradient stream has drained."""

    in_graph = True   # backward + SGD are part of a captured step graph (IterBasedRunner)

    def __init__(self, grad_clip=None):
        if grad_clip is not None:
            raise NotImplementedError("grad_clip is not configured by the in-tree configs")

    def after_train_iter(self, runner):
        from ..hip import streams
        ck = runner.backward(runner.outputs["loss"])
        t0 = runner._tick()
        scale = runner.grad_scale()
        early, late = runner.split_ranges()
        if ck is not None and early:
            # gradients of everything behind the checkpoint are final once the side stream has passed
            # it: update those parameters while the stem / stage-1 weight gradients still run
            for ev in ck:
                torch.cuda.current_stream().wait_event(ev)
            runner._sgd(early, scale, runner.hyper)
            streams.join_side_streams()
            runner._sgd(late, scale, runner.hyper)
        else:
            streams.join_side_streams()
            runner._sgd(runner.active_ranges, scale, runner.hyper)
        # the step cleared exactly the ranges backward wrote: the next zero_grad has nothing to do
        runner.arena.grads_clean = True
        runner.mark("step_end")
        runner._tick("finish+sgd", t0)


class Fp16ArenaOptimizerHook(ArenaOptimizerHook):
    """``optimizer_config = dict(type='Fp16OptimizerHook', loss_scale=...)`` (mmcv's hook, which
    mmseg's fp16 configs name) on the arena SGD: fp16 conv operands in the training step
    (ops.train_precision: forward and data gradient) and a static loss scale S --
    backward is seeded with S and SGD's gradient scale becomes 1 / (world_size * S).  As mmcv's hook
    does in before_run, the model is wrapped for fp16 (its evaluation then runs in fp16 as well) and
    a scaler state found in ``runner.meta['fp16']['loss_scaler']`` (a resumed checkpoint) is restored.
    Only the static form: ``loss_scale='dynamic'`` or a dict are refused (not implemented).
    ``attention``: the model is wrapped for fp16 attention too."""

    def __init__(self, grad_clip=None, loss_scale=512., coalesce=True, bucket_size_mb=-1,
                 distributed=True, attention=False):
        super().__init__(grad_clip)
        from .fp16_utils import LossScaler
        self.loss_scaler = LossScaler(**parse_loss_scale(loss_scale))
        self.attention = attention   # ``fp16 = dict(attention=True)`` of the config (apis.train.optimizer_hook)

    def before_run(self, runner):
        from .fp16_utils import wrap_fp16_model
        if any(isinstance(h, SandwichHook) for h in runner.hooks):
            raise ValueError("fp16 training with use_distillation (sandwich) is not supported")
        wrap_fp16_model(runner.model, attention=self.attention)
        saved = ((runner.meta or {}).get("fp16") or {}).get("loss_scaler")
        if saved is not None:
            self.loss_scaler.load_state_dict(saved)
        runner.train_precision = "fp16"
        runner.loss_scale = self.loss_scaler.loss_scale
        runner.meta = dict(runner.meta or {})
        runner.meta["fp16"] = dict(runner.meta.get("fp16") or {}, loss_scaler=self.loss_scaler.state_dict())


def parse_loss_scale(loss_scale):
    """mmcv's Fp16OptimizerHook ``loss_scale`` -> LossScaler arguments.  A number is a static scale;
    'dynamic' and dicts (dynamic scaling) are recognised and refused: not implemented."""
    if isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float, str, dict)):
        raise ValueError("loss_scale must be a number, 'dynamic' or a dict, got %r" % (loss_scale,))
    if isinstance(loss_scale, (int, float)):
        if not loss_scale > 0 or loss_scale != loss_scale or loss_scale == float("inf"):
            raise ValueError("loss_scale must be a finite positive number, got %r" % (loss_scale,))
        return dict(init_scale=float(loss_scale), mode="static")
    if loss_scale == "dynamic" or isinstance(loss_scale, dict):
        raise NotImplementedError("dynamic loss scaling (loss_scale=%r): only a static loss_scale "
                                  "(a number) is implemented" % (loss_scale,))
    raise ValueError("loss_scale must be a number, 'dynamic' or a dict, got %r" % (loss_scale,))


class TextLoggerHook(Hook):
    def __init__(self, interval=50, by_epoch=False, logger=None, **unused):
        self.interval = interval
        self.logger = logger
        self._t0 = None

    def before_run(self, runner):
        self._t0 = time.time()

    def after_train_iter(self, runner):
        if not self.every_n_iters(runner, self.interval):
            return
        lv = runner.outputs["log_vars"]
        items = ", ".join("%s: %.4f" % (k, float(v)) for k, v in lv.items())
        dt = (time.time() - self._t0) / self.interval
        self._t0 = time.time()
        if runner.train_precision != "fp32" or runner.loss_scale != 1.0:
            items += ", loss_scale: %g" % runner.loss_scale
        if runner.apply_input_shape and runner.input_size is not None:
            items += ", input: %dx%d" % runner.input_size
        msg = "Iter [%d/%d]\tlr: %.3e, arch: %s, time: %.3f, %s" % (
            runner.iter + 1, runner.max_iters, runner.lr, runner.arch_name, dt, items)
        if gdist.rank() == 0:
            (self.logger.info if self.logger else print)(msg)


class CheckpointHook(Hook):
    def __init__(self, interval=-1, by_epoch=False, out_dir=None, **unused):
        self.interval, self.out_dir = interval, out_dir

    def after_train_iter(self, runner):
        if self.interval > 0 and self.every_n_iters(runner, self.interval) and gdist.rank() == 0:
            from .checkpoint import save_checkpoint
            out_dir = self.out_dir or runner.work_dir
            os.makedirs(out_dir, exist_ok=True)
            save_checkpoint(runner.model, os.path.join(out_dir, "iter_%d.pth" % (runner.iter + 1)),
                            optimizer=runner.arena, meta=dict(runner.meta or {}, iter=runner.iter + 1))


class _StepGraph:
    """``keep``: device tensors whose addresses the captured launches carry and that nothing else is
    sure to keep alive for as long as the graph (the chunk tables and the hyper table of a grouped SGD
    step: the arena's table cache may evict them)."""
    __slots__ = ("graph", "static", "outputs", "counters", "keep")

    def __init__(self, graph, static, outputs, counters, keep=()):
        self.graph, self.static, self.outputs, self.counters = graph, static, outputs, counters
        self.keep = list(keep)


class IterBasedRunner:
    """``run(data_loaders, workflow)`` drives ``model.train_step`` for ``max_iters`` iterations."""

    def __init__(self, model, arena, reducer, base_lr=0.01, momentum=0.9, weight_decay=5e-4,
                 max_iters=80000, work_dir=None, logger=None, meta=None, param_groups=None,
                 apply_input_shape=False):
        self.model, self.arena, self.reducer = model, arena, reducer
        # elastic input resolution (config key apply_input_shape): with the flag
        # set_arch remembers the meta's data.input_shape and _train_iter rescales the batch to it;
        # without it the key is carried and nothing reads it
        self.apply_input_shape = bool(apply_input_shape)
        self.input_shape = None        # the current meta's data.input_shape value (flag on only)
        self.input_size = None         # (H, W) of the last step's batch (flag on only: the logger's)
        self.base_lr = self.lr = base_lr
        self.momentum, self.weight_decay = momentum, weight_decay
        # parameter groups (core/optimizer.py build_param_groups; None = one lr / weight decay):
        # group_lr follows the schedule (LrUpdaterHook), group_wd is fixed here
        self.param_groups = param_groups
        self.group_base_lr = self.group_lr = self.group_wd = None
        # the optimizer kind is the arena's (ParamArena.set_optimizer, from cfg.optimizer.type in
        # apis.train.prepare_training); AdamW has the table-driven path only, so it always has groups
        self.optimizer = arena.optimizer
        if self.optimizer == "AdamW" and param_groups is None:
            from .optimizer import ParamGroups
            param_groups = self.param_groups = ParamGroups(
                [(1., 1.)], {n: 0 for n, p in model.named_parameters() if p.requires_grad})
        if param_groups is not None:
            arena.set_param_groups(param_groups.index, len(param_groups))
            self.group_base_lr = param_groups.lrs(base_lr)
            self.group_lr = list(self.group_base_lr)
            self.group_wd = param_groups.weight_decays(weight_decay)
        self.max_iters = max_iters
        self.work_dir, self.logger, self.meta = work_dir, logger, meta
        self.iter = 0
        self.hooks = []
        self.outputs = None
        self.arch_name = "supernet"
        self.active_params = None      # parameters the current subnet uses
        self.trainable_params = None   # ... of those, the ones that receive gradients / updates
        self.active_ranges = None      # merged arena ranges of trainable_params
        self.arch_key = None
        self.arch_meta = None
        self._split_cache = {}
        self.early_steps = 0           # optimizer steps begun inside backward: none (bench.py reports it)
        self.step_events = {} if os.environ.get("GS_STEP_EVENTS") else None
        self._active_cache = {}
        # GS_HOST_PROF=1: accumulate host-side seconds per phase of train_iter (diagnostics)
        self.host_prof = {} if os.environ.get("GS_HOST_PROF") else None
        # ---- step graphs (see train_iter) ----
        # off by default: on ROCm 7.2 hipGraphLaunch spends as much host time per kernel node as the
        # eager path spends per launch (r02: 8.3 ms to launch the 560-node R50 step graph against
        # 8.0 ms of eager host work), so a replay neither frees the host nor closes launch gaps
        self.graphs_enabled = os.environ.get("GS_STEP_GRAPH", "0") == "1"
        self.graphs_paused = False     # e.g. while HIP-event timers are recorded inside the step
        self.max_graphs = int(os.environ.get("GS_STEP_GRAPH_MAX", "8"))
        self._graphs = OrderedDict()   # graph key -> _StepGraph (LRU)
        self._arch_seen = {}           # arch key -> eager steps run with it
        self.hyper = None              # device {lr, momentum, weight_decay, grad_scale} (graphs on)
        self.graph_stats = {"captured": 0, "replayed": 0, "eager": 0}
        self.sandwich = None           # (members, kd_cfg) of THIS iteration, set by SandwichHook
        self.last_checkpoint = None    # the last backward's side-stream checkpoint (see backward)
        # fp16 training (Fp16ArenaOptimizerHook sets both; settable independently): the conv operand
        # precision of every train_iter ('fp32' / 'fp16', ops.train_precision) and the static loss
        # scale S that seeds backward (SGD divides it out: grad_scale)
        self.train_precision = "fp32"
        self.loss_scale = 1.0
        self._loss_seeds = {}
        self.set_arch(None)

    def register_hook(self, hook):
        self.hooks.append(hook)

    # ---- GS_STEP_EVENTS=1 (diagnostics): HIP events at the phase boundaries of every step, on the
    # stream the phase ends on; bench.py prints the mean offsets from the step's start.  Unlike a
    # profiler trace this does not slow the host down, so it shows the real critical path.
    def mark(self, name, stream=None):
        ev = self.step_events
        if ev is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream if stream is not None else torch.cuda.current_stream())
        ev.setdefault(name, []).append(e)

    def step_event_summary(self):
        """{phase: mean ms from 'step_begin'} over the recorded steps (call after a synchronize)."""
        ev = self.step_events
        if not ev or "step_begin" not in ev:
            return {}
        n = len(ev["step_begin"])
        out = {}
        for name, lst in ev.items():
            if name == "step_begin" or len(lst) != n:
                continue
            out[name] = sum(b.elapsed_time(e) for b, e in zip(ev["step_begin"], lst)) / n
        return out

    def call_hook(self, name):
        for h in self.hooks:
            getattr(h, name)(self)

    def set_arch(self, meta):
        """Apply a sampled meta (None = keep the current, max, architecture)."""
        if meta is not None:
            shape = meta.get(INPUT_SHAPE_KEY) if self.apply_input_shape else None
            if shape is not None:
                parse_input_shape(shape)      # (refused at first sight, before anything is switched)
            self.model.manipulate_arch(fold_dict(meta)["arch"])
            self.arch_name = meta.get("name", "random")
            self.arch_key = arch_key(meta)
            self.arch_meta = meta
            self.input_shape = shape
        else:
            self.arch_key = ("current",)
            self.input_shape = None
        self.refresh_active()

    def refresh_active(self, force=False):
        """Recompute the active parameter sets from the model's CURRENT arch state.  Frozen
        parameters (frozen_stages / frozen_layers / norm_cfg requires_grad=False) are left out of
        the zero / all-reduce / SGD ranges: torch.optim.SGD skips parameters without a gradient,
        so they must neither decay nor move (gaiaseg/models/backbones/dynamic_resnet.py:304-334).
        The sets of a named / sampled subnet are cached by its arch key (the module walk costs
        ~0.4 ms per step otherwise); ``force`` drops the cache (requires_grad flags were edited)."""
        key = self.cache_key
        if force:
            self._active_cache.clear()
        hit = self._active_cache.get(key) if key is not None else None
        if hit is None:
            active = self.model.active_parameters()
            hit = (active, [p for p in active if p.requires_grad])
            if key is not None:
                if len(self._active_cache) > 1024:
                    self._active_cache.clear()
                self._active_cache[key] = hit
        self.active_params, self.trainable_params = hit
        self.active_ranges = self.arena.ranges_for(self.trainable_params, key)
        if self.arena.groups is not None:
            # chunk tables are built and uploaded here, never inside a graph capture
            for r in (self.active_ranges,) + tuple(self.split_ranges()):
                self.arena.chunk_table(r)

    @property
    def cache_key(self):
        """The arch key the per-subnet caches (active sets, ranges, gradient buckets) are filed
        under; None for an architecture nobody named (set_arch(None)): not cached."""
        return self.arch_key if self.arch_key != ("current",) else None

    # what _sgd hands to arena.sgd_step: one value, or one per parameter group
    @property
    def opt_lr(self):
        return self.lr if self.group_lr is None else self.group_lr

    @property
    def opt_wd(self):
        return self.weight_decay if self.group_wd is None else self.group_wd

    def split_ranges(self):
        """(early, late) parts of active_ranges: `late` covers the parameters whose weight gradients
        are produced last in backward (backbone.late_gradient_parameters), `early` the rest."""
        key = self.cache_key
        cached = self._split_cache.get(key) if key is not None else None
        if cached is not None:
            return cached
        late_fn = getattr(getattr(self.model, "backbone", None), "late_gradient_parameters", None)
        late_ids = {id(p) for p in late_fn()} if late_fn is not None else set()
        early_p = [p for p in self.trainable_params if id(p) not in late_ids]
        late_p = [p for p in self.trainable_params if id(p) in late_ids]
        out = (self.arena.ranges_for(early_p), self.arena.ranges_for(late_p))
        if key is not None:
            self._split_cache[key] = out
        return out

    # ------------------------------------------------------------------------------------------
    # Step graphs.  A training step of a given subnet on a given batch shape is a fixed sequence of
    # ~600-1100 kernel launches (forward, backward, SGD) whose only step-dependent inputs are the
    # batch and the learning rate.  For subnets that come back (the named anchors of the train
    # sampler, or any subnet seen before) the whole step is captured ONCE into a HIP graph
    # (torch.cuda.CUDAGraph: stream capture of the launches the C-ABI makes on torch's current
    # stream and on the weight-gradient side stream) and replayed afterwards: the batch is copied
    # into the graph's static input tensors, lr / momentum / weight decay sit in a 16-byte device
    # buffer the SGD kernel reads (gs_sgd_step_hyper), and one graph launch replaces the host-side
    # walk over the modules.  Same kernels, same order, same results as the eager step (bit-identical:
    # tests/test_runner_gpu.py).  Never-repeating random subnets, multi-rank runs (RCCL launches are
    # left out of capture), SyncBN groups and diagnostic traces keep the eager path.
    # MEASURED (r02, MI355X, ROCm 7.2): the graph launch itself costs the host ~15 us per kernel node,
    # i.e. as much as the eager path; R50 192.9 img/s replayed vs 198.5 eager, the sampled mix loses
    # 40 % (switching between large graphs).  The feature is therefore OPT-IN (GS_STEP_GRAPH=1).
    # ------------------------------------------------------------------------------------------
    def _graph_key(self, data_batch):
        from ..hip import ops
        if (not self.graphs_enabled or self.graphs_paused or self.arch_key is None
                or self.arch_key == ("current",) or gdist.world_size() != 1
                or ops.RELU_TRACE is not None or ops.POOL_TRACE is not None or ops.TIMER is not None
                or not getattr(self.model, "step_graph_capturable", True)):
            return None
        sig = []
        for k in sorted(data_batch):
            v = data_batch[k]
            if torch.is_tensor(v):
                if not v.is_cuda:
                    return None
                sig.append((k, tuple(v.shape), v.dtype))
        # (a step captured in fp32 must never be replayed in fp16, nor one scaled by another S)
        # (nor a step captured under another grouping: the arena counts its set_param_groups calls)
        grouping = None if self.arena.groups is None else (self.arena.group_epoch, self.arena.groups)
        # (nor one captured with the fp32 attention kernels under the fp16 ones, or the reverse)
        attention = tuple(bool(m.fp16_attention) for m in self.model.modules() if hasattr(m, "fp16_attention"))
        return (self.arch_key, tuple(sig), self.model.training, grouping, attention, self.train_precision,
                self.loss_scale)

    def _apply_input_shape(self, data_batch):
        """The batch at the current meta's data.input_shape (flag on; a copy: the caller's batch is
        left alone).  The result's tensor shapes are part of _graph_key, so every (subnet,
        resolution) pair gets a step graph of its own."""
        if self.input_shape is None:
            self.input_size = tuple(int(d) for d in data_batch["img"].shape[-2:])
            return data_batch
        data_batch, self.input_size = rescale_batch(data_batch, self.input_shape)
        return data_batch

    def grad_scale(self):
        """SGD's gradient scale: the all-reduce sums world_size ranks' gradients of the loss times S."""
        return 1.0 / (gdist.world_size() * self.loss_scale)

    def loss_seed(self, loss):
        """The device scalar S that seeds backward (one per device: graph captures reuse it)."""
        key = (loss.device, loss.dtype, self.loss_scale)
        t = self._loss_seeds.get(key)
        if t is None:
            t = self._loss_seeds[key] = torch.full((), self.loss_scale, dtype=loss.dtype, device=loss.device)
        return t

    def _write_hyper(self):
        """lr / momentum / weight decay / gradient scale of THIS step -> the device buffer."""
        from ..hip import lib as _lib
        from ..hip.runtime import current_stream_ptr
        if self.hyper is None:
            self.hyper = torch.zeros(4, dtype=torch.float32, device=self.arena.flat_param.device)
        if self.optimizer == "AdamW":      # (its own fp64 table; ``hyper`` only says "written")
            self.arena.write_adamw_hyper(self.group_lr, self.group_wd, self.grad_scale())
            return
        _lib.check(_lib.load().gs_sgd_set_hyper(self.hyper.data_ptr(), self.lr, self.momentum,
                                                self.weight_decay, self.grad_scale(),
                                                current_stream_ptr()), "gs_sgd_set_hyper")
        if self.group_lr is not None:
            self.arena.write_group_hyper(self.group_lr, self.group_wd, self.momentum, self.grad_scale())

    def _tick(self, key=None, since=0.0):
        """GS_HOST_PROF: the host clock (0.0 with the profile off); with ``key`` the seconds since
        ``since`` are added to host_prof[key]."""
        if self.host_prof is None:
            return 0.0
        now = time.perf_counter()
        if key is not None:
            self.host_prof[key] = self.host_prof.get(key, 0.0) + (now - since)
        return now

    def _begin_step(self):
        """Before a subnet's forward: its gradients zero and marked dirty, the reducer armed."""
        self.arena.zero_grad(self.active_ranges, trust_clean=True)   # (a no-op after a clearing optimizer step)
        self.arena.grads_clean = False
        self.reducer.begin(self.trainable_params, self.cache_key)

    def backward(self, loss):
        """``loss.backward()`` (seeded with the static loss scale) under streams.deferred_join, then the
        branch streams joined and the reducer finished.  Returns the side stream's checkpoint events
        or None (kept in ``last_checkpoint``); joining the side stream is left to the caller, which
        may step the early instalment first (ArenaOptimizerHook)."""
        from ..hip import streams
        t0 = self._tick()
        self.mark("fwd_end")
        with streams.deferred_join() as dj:
            if self.loss_scale != 1.0:
                loss.backward(gradient=self.loss_seed(loss))   # (static loss scale S)
            else:
                loss.backward()
        t1 = self._tick("backward", t0)
        self.mark("bwd_end_main")
        side = streams.side_stream(self.arena.device)
        if side is not None:
            self.mark("bwd_end_side0", side)
        streams.join_branch_streams()  # (auxiliary head / shortcut work on the branch stream)
        self.reducer.finish()
        self._tick("finish+sgd", t1)
        self.last_checkpoint = dj.checkpoint
        return dj.checkpoint

    def _sgd(self, ranges, grad_scale, hyper=None):
        """One fused optimizer step on ``ranges`` that clears the gradients it consumed."""
        if self.optimizer == "AdamW":
            self.arena.adamw_step(ranges, self.opt_lr, self.opt_wd, grad_scale, True, hyper=hyper)
            return
        self.arena.sgd_step(ranges, self.opt_lr, self.momentum, self.opt_wd, grad_scale, True,
                            hyper=hyper)

    def _after_hooks(self, in_graph):
        for h in self.hooks:
            if bool(getattr(h, "in_graph", False)) == in_graph:
                h.after_train_iter(self)

    def _capture_step(self, key, data_batch):
        """Capture forward + backward + SGD of the current subnet into a graph, then run it once."""
        from ..hip import runtime, streams
        dev = self.arena.flat_param.device
        static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data_batch.items()}
        streams.reserve_workspaces(dev)   # no workspace may be (re)allocated inside the capture
        graph = torch.cuda.CUDAGraph()
        runtime.CAPTURE_LOG = []
        self.arena.capture_refs = []   # (the graph entry owns the tables its SGD launches name)
        try:
            with torch.cuda.graph(graph):
                self.outputs = self.model.train_step(static, None)
                self._after_hooks(True)
            counters, keep = runtime.CAPTURE_LOG, self.arena.capture_refs
        finally:
            runtime.CAPTURE_LOG = None
            self.arena.capture_refs = None
        entry = _StepGraph(graph, static, self.outputs, counters, keep)
        self._graphs[key] = entry
        while len(self._graphs) > self.max_graphs:
            self._graphs.popitem(last=False)
        self.graph_stats["captured"] += 1
        graph.replay()                 # the capture only recorded the step: this performs it
        return entry

    def _step(self, capture_key, data_batch):
        """One training step outside a replay: eager, or (``capture_key``) captured into a step graph
        and run once.  Returns the host clock after _begin_step and after the forward / the capture."""
        self._begin_step()
        t2 = self._tick()
        if capture_key is not None:
            self._capture_step(capture_key, data_batch)
            return t2, self._tick()
        self.outputs = self.model.train_step(data_batch, None)
        t3 = self._tick()
        self._after_hooks(True)
        self.graph_stats["eager"] += 1
        return t2, t3

    def _replay_step(self, entry, data_batch):
        for k, v in entry.static.items():
            if torch.is_tensor(v):
                v.copy_(data_batch[k], non_blocking=True)
        entry.graph.replay()
        for m in entry.counters:       # host-side effects of the step that the graph cannot carry
            m._nbt_pending = getattr(m, "_nbt_pending", 0) + 1
        self.outputs = entry.outputs
        self.arena.grads_clean = True  # (the captured SGD step clears the gradients it consumed)
        self.graph_stats["replayed"] += 1

    def prepare_graphs(self, metas, data_batch):
        """Capture the step graphs of the given subnets ahead of time (e.g. the sampler's anchors at
        start-up) instead of at their first occurrence.  Every capture performs one real training
        step on ``data_batch``; the architecture in place before the call is restored."""
        keep = self.arch_meta
        done = 0
        for meta in metas:
            self.set_arch(meta)
            batch = self._apply_input_shape(data_batch) if self.apply_input_shape else data_batch
            gkey = self._graph_key(batch)
            if gkey is None or gkey in self._graphs:
                continue
            for capture in ((False, True) if self.graph_stats["eager"] == 0 else (True,)):
                self._write_hyper()
                self._step(gkey if capture else None, batch)
            done += 1
        if keep is not None:
            self.set_arch(keep)
        return done

    # The training step runs on a HIGH-PRIORITY stream (GS_TRAIN_PRIORITY=0: on the caller's stream):
    # the weight-gradient and branch streams keep normal priority, so when both have workgroups ready
    # the dispatcher serves the chain every later kernel waits for — data gradients, BatchNorm passes —
    # first and the weight gradients fill in behind.  The gradient exchange runs at high priority too:
    # bench.py and tools/train_supernet.py create the RCCL process group with high-priority streams
    # under the same switch, so a bucket's all-reduce is dispatched when it is issued.  Same
    # kernels, same order on every stream, same results (tests/test_runner_gpu.py); r04 A/B on the
    # sampled mix: 166.4 -> 169.9 images/s (five interleaved runs each, the two sets do not overlap),
    # R50 unchanged (profiles/r04_stream_experiments.md).
    # The stream becomes the CURRENT stream of the calling thread at the first train_iter and stays it
    # (after waiting for what the caller had queued on its own stream): going back and forth between
    # the legacy default stream and this one every step made every launch 3x as expensive on the host
    # (45 us per conv + BN call instead of 15: measured, 166 -> 83 images/s).
    TRAIN_PRIORITY = os.environ.get("GS_TRAIN_PRIORITY", "1") != "0"

    def _enter_priority_stream(self):
        dev = self.arena.device
        if not self.TRAIN_PRIORITY or dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
            return
        hp = self.__dict__.get("_hp_stream")
        if hp is None:
            hp = self._hp_stream = torch.cuda.Stream(device=dev, priority=-1)
        cur = torch.cuda.current_stream(dev)
        if cur != hp:
            hp.wait_stream(cur)
            torch.cuda.set_stream(hp)

    def train_iter(self, data_batch):
        self._enter_priority_stream()
        if self.train_precision == "fp32":
            return self._train_iter(data_batch)
        from ..hip import ops
        with ops.train_precision(self.train_precision):   # (fp32 again on return or raise)
            return self._train_iter(data_batch)

    def _train_iter(self, data_batch):
        t0 = self._tick()
        self.mark("step_begin")
        if not self.model.training:   # (a full module walk: ~1.5 ms of host time per call)
            self.model.train()
        self.call_hook("before_train_iter")
        if self.sandwich is not None:
            members, kd_cfg = self.sandwich
            self.sandwich = None
            self._sandwich_iter(data_batch, members, kd_cfg)
            self._after_hooks(False)
            self.iter += 1
            return self.outputs
        if self.apply_input_shape:
            data_batch = self._apply_input_shape(data_batch)
        t1 = self._tick()
        gkey = self._graph_key(data_batch)
        if self.graphs_enabled and gdist.world_size() == 1:
            self._write_hyper()
        entry = self._graphs.get(gkey) if gkey is not None else None
        if entry is not None:
            self._graphs.move_to_end(gkey)
            self._replay_step(entry, data_batch)
            t2, t3 = t1, self._tick()
        else:
            # capture at first sight what is known to come back (named anchors), anything else the
            # second time it shows up; the very first step of a process always runs eagerly (module
            # loading and lazily created handles must not happen inside a capture)
            known = self.arch_name != "random" or self._arch_seen.get(self.arch_key, 0) > 0
            capture = gkey is not None and known and self.graph_stats["eager"] > 0
            t2, t3 = self._step(gkey if capture else None, data_batch)
            if gkey is not None and not capture:
                self._arch_seen[self.arch_key] = self._arch_seen.get(self.arch_key, 0) + 1
                if len(self._arch_seen) > 4096:
                    self._arch_seen.clear()
        self._after_hooks(False)
        prof = self.host_prof
        if prof is not None:
            t4 = time.perf_counter()
            for k, v in (("hooks_before", t1 - t0), ("zero+begin", t2 - t1), ("forward", t3 - t2),
                         ("backward+opt", t4 - t3)):
                prof[k] = prof.get(k, 0.0) + v
            prof["iters"] = prof.get("iters", 0) + 1
        self.iter += 1
        return self.outputs

    # In-place distillation (SandwichHook): US-Nets' sandwich rule as the reference's train_step
    # ("dynamic_encoder_decoder-distill-backup (1).py":52-64) + an optimizer that steps once per
    # iteration (the reference's runner lived in the absent gaiavision package: DESIGN.md §15).
    # Every member runs forward + backward (gradient exchange inside its own backward: all-reduce is
    # linear), then its gradients are MOVED into the arena's accumulation buffer (the weight-gradient
    # kernels overwrite, they cannot add); after the last member the buffer goes back into the
    # gradients over the union of the members' ranges and one fused SGD step clears them again.
    # Eager only: no step graphs, no early / split SGD instalments.
    def _sandwich_iter(self, data_batch, members, kd_cfg):
        from ..hip import streams
        total, log_vars, union, names = None, OrderedDict(), [], []
        teacher = None
        n_random = 0
        for i, meta in enumerate(members):
            self.set_arch(meta)
            name = meta.get("name")
            if name is None:
                name, n_random = "random%d" % n_random, n_random + 1
            names.append(name)
            self._begin_step()
            if i == 0:
                out = self.model.train_step(data_batch, None, return_logits=True)
                teacher = (out["logits"], out["aux_logits"])
            else:
                out = self.model.train_step(data_batch, None, teacher_logits=teacher[0],
                                            aux_teacher_logits=teacher[1], **kd_cfg)
            self.backward(out["loss"])
            streams.join_side_streams()    # (every stream joined: the member's gradients are final)
            self.arena.accumulate(self.active_ranges, into="buffer")
            self.arena.grads_clean = True          # (the move left zeros behind)
            union = _ranges_union(union, self.active_ranges)
            loss, logged = out["loss"].detach(), out["log_vars"]["loss"]   # (local / rank-averaged)
            total = (loss, logged) if total is None else (total[0] + loss, total[1] + logged)
            for k, v in out["log_vars"].items():
                log_vars["%s.%s" % (name, k)] = v
        self.arena.accumulate(union, into="grad")
        self.arena.grads_clean = False
        self._sgd(union, 1.0 / gdist.world_size())
        self.arena.grads_clean = True
        self.arch_name = "sandwich"
        log_vars["loss"] = total[1]
        self.outputs = dict(loss=total[0], log_vars=log_vars, num_samples=len(data_batch["img_metas"]),
                            members=names, teacher_logits=teacher)
        return self.outputs

    def run(self, data_loaders, workflow=(("train", 1),), max_iters=None):
        if max_iters is not None:
            self.max_iters = max_iters
        self.call_hook("before_run")
        loader = iter(data_loaders[0])
        while self.iter < self.max_iters:
            try:
                batch = next(loader)
            except StopIteration:
                loader = iter(data_loaders[0])
                batch = next(loader)
            self.train_iter(batch)
        self.call_hook("after_run")

    def resume(self, checkpoint):
        from .checkpoint import load_checkpoint
        ck = load_checkpoint(self.model, checkpoint, strict=True)
        if "optimizer" in ck:
            self.arena.load_state_dict(ck["optimizer"], logger=self.logger)
        self.iter = ck.get("meta", {}).get("iter", 0)
        if "fp16" in ck.get("meta", {}):   # the loss scaler's state (Fp16ArenaOptimizerHook.before_run)
            self.meta = dict(self.meta or {}, fp16=ck["meta"]["fp16"])

    def load_checkpoint(self, checkpoint):
        from .checkpoint import load_checkpoint
        load_checkpoint(self.model, checkpoint, strict=False)
