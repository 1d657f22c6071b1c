"""finetune_model_space — the loop of the reference's tools/finetune_supernet.py:264-358 (fast-finetune:
train every selected subnet for a few iterations from the supernet's weights, then evaluate it) on
ONE resident supernet.

The reference calls train_segmentor once per subnet on the same model object (each call re-wraps
it in DDP and rebuilds the optimizer and the loaders) and reads ``latest.pth`` back before testing.
Here the supernet is snapshotted once on the device (S0: the parameter arena and every module
buffer) and every subnet's turn starts by restoring S0, so a turn is a function of (S0, subnet,
seed) only -- the rows do not depend on the order or the company a subnet is finetuned in, which the
reference cannot promise: there subnet k starts from the weights subnet k-1 left behind.
DESIGN.md section 19 lists what S0 holds, what a turn restores and the deviations.
"""
import time

import torch

from ..core import dist as gdist
from ..core.dynamic import fold_dict
from ..core.input_shape import INPUT_SHAPE_KEY
from ..core.model_space import _listify, build_model_sampler, parse_input_shape
from .train import (build_dataloader, check_lr_policy, optimizer_hook, prepare_training,
                    run_training, set_random_seed)

METRICS = ("mIoU", "mAcc", "aAcc")


def anchor_sampler_cfg(meta, index=0):
    """The one-anchor sampler config of a flat meta, the form the reference builds at
    tools/finetune_supernet.py:283-288: ``{'name': <name>, **meta}`` -- a name the meta carries wins
    over the row index.  Tuples (model-space rows) become lists, the form manipulate_arch takes."""
    return dict(type="anchor", anchors=[{"name": str(index), **_listify(dict(meta))}])


def finetune_row(meta, result, metric_tag="finetune"):
    """The output row: the meta with every column it has (other metric tags included) plus
    ``metric.<tag>.mIoU`` / ``.mAcc`` / ``.aAcc``."""
    row = dict(meta)
    for k in METRICS:
        row["metric.%s.%s" % (metric_tag, k)] = result[k]
    return row


def check_finetune_cfg(cfg, metas):
    """Everything fast-finetune refuses, checked before the model is touched; returns nothing."""
    if cfg.get("use_distillation", False):
        raise ValueError("use_distillation with fast-finetune (one anchor per run: there is no "
                         "sandwich to distil in) is not supported")
    if (cfg.get("caliberate_bn") or {}).get("use_minibatch_stats", False):
        raise ValueError("caliberate_bn.use_minibatch_stats with fast-finetune is not supported: it "
                         "drops the running statistics for good, and the subnets after the first "
                         "could not be restored")
    if (cfg.get("caliberate_bn") or {}).get("recalibrate") is not None:
        raise ValueError("caliberate_bn.recalibrate with fast-finetune is not supported: a finetuned "
                         "subnet's BatchNorm statistics are already its own; re-calibration belongs to "
                         "tools/test_supernet.py")
    if not metas:
        raise ValueError("fast-finetune: no subnet to finetune (empty metas)")
    # grad_clip / dynamic loss scale / a non-bool fp16.attention: refused here
    optimizer_hook(cfg.get("optimizer_config"), cfg.get("fp16"))
    if cfg.get("apply_input_shape", False):          # a scale no batch can take: refused here
        for meta in metas:
            if meta.get(INPUT_SHAPE_KEY) is not None:
                parse_input_shape(meta[INPUT_SHAPE_KEY])
    check_lr_policy(cfg)


class SupernetSnapshot:
    """S0: a device-side copy of the parameter arena and of every module buffer, and the host-side
    state a run changes (arch, training mode, fp16_enabled and fp16_attention flags).  ``restore`` is
    device copies only."""

    def __init__(self, model, arena):
        self.model, self.arena = model, arena
        self._flush(model)             # pending num_batches_tracked counts belong to S0
        with torch.no_grad():
            self.flat_param = arena.flat_param.clone()
            self.buffers = [(b, b.clone()) for b in model.buffers()]
        self.arch = {"backbone": {k: v for k, v in model.backbone.state_dict_of_arch().items()
                                  if v is not None}}
        self.training = model.training
        self.fp16 = [(m, m.fp16_enabled) for m in model.modules() if hasattr(m, "fp16_enabled")]
        self.fp16_attention = [(m, m.fp16_attention) for m in model.modules() if hasattr(m, "fp16_attention")]

    @staticmethod
    def _flush(model):
        for m in model.modules():
            if hasattr(m, "flush_counters"):
                m.flush_counters()

    def restore(self, host_state=False):
        """Parameters and buffers back to S0 bit for bit, momentum / gradient / accumulation arenas
        zero (``grads_clean`` truthful), per-module caches of old buffers dropped.  ``host_state``:
        also the arch and the training mode found at snapshot time.  The fp16_enabled and fp16_attention
        flags (set by the fp16 hook of a run) go back either way."""
        a = self.arena
        with torch.no_grad():
            a.flat_param.copy_(self.flat_param)
            for b, saved in self.buffers:
                b.copy_(saved)
            a.reset_optimizer_state()    # (momentum; AdamW: both moments and the step counters)
            a.flat_grad.zero_()
            if a.flat_acc is not None:
                a.flat_acc.zero_()
        a.grads_clean = True
        for m in self.model.modules():
            d = m.__dict__
            d.pop("_bnp_cache", None)
            if "_nbt_pending" in d:      # counted by the run that just ended: not part of S0
                d["_nbt_pending"] = 0
        for m, flag in self.fp16:
            m.fp16_enabled = flag
        for m, flag in self.fp16_attention:
            m.fp16_attention = flag
        if host_state:
            self.model.manipulate_arch(self.arch)
            self.model.train(self.training)


def _restart(loader):
    """The train data from its beginning: loaders know how (``restart``); a list of batches is
    iterated from its first element by the runner anyway."""
    fn = getattr(loader, "restart", None)
    if fn is not None:
        fn()


def finetune_model_space(model, metas, cfg, train_data, val_loader, num_batches,
                         metric_tag="finetune", validate=False, seed=0, logger=None, on_subnet=None):
    """Fast-finetune every subnet of ``metas`` from the weights ``model`` holds and evaluate it.

    ``model``: the supernet on the device with the checkpoint loaded; ``metas``: flat dotted metas
    (ModelSpace.rows); ``train_data``: a dataset config or an iterable of batches, as train_segmentor
    takes; ``val_loader`` / ``num_batches``: as apis.test.test_model_space.  For each meta, in order:
    restore S0, ``set_random_seed(seed)`` and restart the train data, train ``cfg.runner.max_iters``
    iterations exactly as train_segmentor trains the anchor ``{'name': <name>, **meta}`` (same
    hooks from the same config keys; no CheckpointHook, no checkpoint read), evaluate in eval mode
    under the subnet's arch, and emit the row (finetune_row).  With ``cfg.apply_input_shape`` a row
    that carries ``data.input_shape`` is trained and evaluated at that size.
    ``on_subnet(row, model)`` runs while the model still holds the finetuned weights.  Afterwards the model is S0 again, with the arch, the
    training mode and the fp16_enabled flags it came with.

    ``optimizer.lr = 0`` makes it a calibration-only run: no parameter moves, the BatchNorm running
    statistics of the subnet's active slices are re-estimated on the train data.

    Returns the rows (identical on every rank)."""
    from ..core.evaluation import check_tta_input_shape, evaluate_model
    metas = list(metas or ())
    check_finetune_cfg(cfg, metas)
    check_tta_input_shape(val_loader, cfg.get("apply_input_shape", False))
    log = (logger.info if logger is not None else print) if gdist.rank() == 0 else (lambda msg: None)

    apply_input_shape = bool(cfg.get("apply_input_shape", False))
    model, arena, reducer, param_groups = prepare_training(model, cfg)
    snap = SupernetSnapshot(model, arena)
    train_loader = build_dataloader(train_data, cfg.data["samples_per_gpu"], seed=cfg.get("seed") or 0,
                                    device=arena.device,
                                    workers_per_gpu=cfg.data.get("workers_per_gpu", 2),
                                    device_cache_gb=cfg.data.get("device_cache_gb"))
    rows, stream = [], None
    try:
        for i, meta in enumerate(metas):
            t0 = time.perf_counter()
            snap.restore()
            set_random_seed(seed)
            _restart(train_loader)
            sampler_cfg = anchor_sampler_cfg(meta, i)
            anchor = sampler_cfg["anchors"][0]
            opt_hook = optimizer_hook(cfg.get("optimizer_config"), cfg.get("fp16"))   # (a fresh loss-scaler state)
            timing = {}

            def before_run(runner, timing=timing):
                if stream is not None:      # one high-priority training stream for the whole space
                    runner._hp_stream = stream
                torch.cuda.synchronize(arena.device)
                timing["train_begin"] = time.perf_counter()

            runner = run_training(model, arena, reducer, param_groups,
                                  build_model_sampler(sampler_cfg), build_model_sampler(sampler_cfg),
                                  train_loader, cfg, opt_hook, validate=validate, logger=logger,
                                  val_loader=val_loader, eval_num_batches=num_batches,
                                  checkpoints=False, before_run=before_run)
            stream = runner.__dict__.get("_hp_stream", stream)
            torch.cuda.synchronize(arena.device)
            t1 = time.perf_counter()
            model.eval()
            model.manipulate_arch(fold_dict(anchor)["arch"])
            res = evaluate_model(model, val_loader, num_batches, model.num_classes,
                                 input_shape=anchor.get(INPUT_SHAPE_KEY) if apply_input_shape else None)
            t2 = time.perf_counter()
            row = finetune_row(meta, res, metric_tag)
            rows.append(row)
            t3 = time.perf_counter()
            if on_subnet is not None:
                on_subnet(row, model)
            train_s, eval_s = t1 - timing["train_begin"], t2 - t1
            log("subnet %d/%d %s: mIoU %.4f mAcc %.4f aAcc %.4f (train %.3f s for %d iters, eval %.3f s, "
                "rest of the turn %.3f s)" % (i + 1, len(metas), anchor["name"], res["mIoU"], res["mAcc"],
                                              res["aAcc"], train_s, runner.iter, eval_s,
                                              (t3 - t0) - train_s - eval_s))
            del runner
    finally:
        snap.restore(host_state=True)
    return rows
