"""train_segmentor — host-side mirror of gaiaseg/apis/train.py:47-186.

Same call contract (model, train_sampler, val_sampler, dataset, cfg, distributed, validate,
timestamp, meta) and the same feature switches read with cfg.get (manipulate_arch :142,
lr_scaler :103-113, resume_from / load_from :172-175).  What differs by design:
  * the model is not wrapped in MMDistributedDataParallel: parameters and gradients live in flat
    arenas and a bucketed RCCL all-reduce over slices of the gradient arena is driven by the
    backward tape (core/dist.py);
  * the optimizer is a fused flat-arena kernel: SGD (the in-tree ResNet configs) or AdamW
    (cfg.optimizer.type, core/optimizer.py; anything else is refused);
  * datasets: the reference's CityscapesDataset19 is not defined anywhere and
    no dataset exists offline, so ``type='SyntheticSegDataset'`` (seeded tensors of the pipeline's
    output shapes) is the built-in loader; any iterable of
    dict(img, img_metas, gt_semantic_seg) batches is accepted.
"""
import random

import numpy as np
import torch

from ..core import dist as gdist
from ..core.optimizer import build_param_groups, check_optimizer_cfg
from ..core.param_arena import ParamArena
from ..core.runner import (ArenaOptimizerHook, CheckpointHook, FixedLrUpdaterHook,
                           Fp16ArenaOptimizerHook, IterBasedRunner, ManipulateArchHook,
                           PolyLrUpdaterHook, SANDWICH_INPUT_SHAPE, SandwichHook, TextLoggerHook,
                           check_sandwich_model)
from ..core.synthetic import SyntheticLoader


def set_random_seed(seed, deterministic=False):
    """gaiaseg/apis/train.py:30-45.  (The HIP kernels are bit-reproducible regardless of
    ``deterministic``: no float atomics are used anywhere on the path.)"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def sandwich_train_sampler(cfg):
    """In-place distillation's train sampler (tools/train_supernet.py:180-187): with
    ``use_distillation`` the config names ``max_net``, ``min_net`` and ``random_subnet`` samplers and
    the train sampler becomes concat[max_net, min_net, random_subnet x sample_subnet_num (default 3)].
    (The reference reads ``cfg.get(sample_subnet_num, 3)`` -- an undefined name -- meaning the key.)"""
    assert cfg.get("max_net", False)
    assert cfg.get("min_net", False)
    assert cfg.get("random_subnet", False)
    sampler = dict(type="concat", model_samplers=[cfg.max_net, cfg.min_net])
    for _ in range(cfg.get("sample_subnet_num", 3)):
        sampler["model_samplers"].append(cfg.random_subnet)
    return sampler


def build_dataloader(dataset_cfg, samples_per_gpu, seed=0, device="cuda", num_classes=19,
                     workers_per_gpu=2, train=True, device_cache_gb=None, rank=None, world=None):
    """mmseg ``build_dataset`` + ``build_dataloader(..., dist, seed, drop_last=True)``
    (gaiaseg/apis/train.py:74-84, tools/train_supernet.py:197) for this path: a config dict naming a
    registered file-backed dataset (``CityscapesDataset19`` of the in-tree configs, ``CityscapesDataset``,
    ``CustomDataset``) becomes a loader whose transforms run on the GPU; ``SyntheticSegDataset`` gives
    the seeded synthetic batches; anything else that is already an iterable of batches passes through
    (a list of batches -- dicts with an ``img`` and no ``type`` -- included).  ``rank`` / ``world``:
    the shard this loader reads instead of the process's own (core/bn_calibration.py: every rank
    reads rank 0 of 1)."""
    rank = gdist.rank() if rank is None else rank
    world = gdist.world_size() if world is None else world
    if isinstance(dataset_cfg, (list, tuple)) and dataset_cfg and all(
            isinstance(b, dict) and "img" in b and "type" not in b for b in dataset_cfg):
        return dataset_cfg
    if isinstance(dataset_cfg, (list, tuple)):
        if len(dataset_cfg) != 1:
            raise NotImplementedError("concatenated datasets (%d entries)" % len(dataset_cfg))
        dataset_cfg = dataset_cfg[0]
    if isinstance(dataset_cfg, dict):
        t = dataset_cfg.get("type")
        if t == "SyntheticSegDataset":
            return SyntheticLoader(samples_per_gpu, tuple(dataset_cfg["size"]),
                                   dataset_cfg.get("num_classes", num_classes), seed=seed,
                                   rank=rank, device=device)
        from ..datasets import (DATASETS, FileBatchLoader, FileEvalLoader, FileTtaEvalLoader,
                                build_dataset, eval_pipeline_kwargs, train_pipeline_kwargs,
                                tta_num_views, tta_pipeline_kwargs)
        if t not in DATASETS:
            raise NotImplementedError("dataset type %r is not registered (have %s and "
                                      "SyntheticSegDataset)" % (t, sorted(DATASETS.module_dict)))
        ds = build_dataset(dataset_cfg)
        # decoded uint8 samples kept in HBM (``data.device_cache_gb``, a key of this build; None = the
        # loaders' defaults, 0 = off)
        extra = {} if device_cache_gb is None else dict(device_cache_bytes=int(device_cache_gb * (1 << 30)))
        if train:
            return FileBatchLoader(ds, samples_per_gpu, train_pipeline_kwargs(ds.pipeline),
                                   workers_per_gpu=workers_per_gpu, seed=seed, rank=rank,
                                   world=world, device=device, **extra)
        common = dict(workers_per_gpu=workers_per_gpu, rank=rank, world=world, device=device, **extra)
        if wants_tta(ds.pipeline):
            # multi-scale / flip test-time augmentation: every batch carries all views.  (A ladder
            # of one view over a fixed scale is the single-view loader's job.)
            tk = tta_pipeline_kwargs(ds.pipeline)
            if tta_num_views(tk) > 1 or tk["scales"] is None:
                return FileTtaEvalLoader(ds, samples_per_gpu, tk, **common)
            return FileEvalLoader(ds, samples_per_gpu, tk["scales"][0], tk["mean"], tk["std"],
                                  tk["to_rgb"], **common)
        tk = eval_pipeline_kwargs(ds.pipeline)
        return FileEvalLoader(ds, samples_per_gpu, tk["img_scale"], tk["mean"], tk["std"], tk["to_rgb"],
                              **common)
    return dataset_cfg  # already an iterable of batches


def wants_tta(pipeline):
    """Does a val / test transform list ask for what the single-view translation
    (eval_pipeline_kwargs) refuses: flipped views, ``img_ratios`` or a list of scales?"""
    for t in pipeline:
        if t.get("type") == "MultiScaleFlipAug":
            scale = t.get("img_scale")
            return bool(t.get("flip", False) or t.get("img_ratios") is not None or scale is None
                        or isinstance(scale, list))
    return False


def optimizer_hook(optimizer_config, fp16=None):
    """``cfg.optimizer_config`` -> the arena optimizer hook (mmcv's register_training_hooks builds
    the hook it names).  ``type='Fp16OptimizerHook'`` turns on fp16 training with its ``loss_scale``
    (core/runner.py Fp16ArenaOptimizerHook); any other (or no) type is the fp32 OptimizerHook.  A
    top-level ``fp16`` key alone means fp16 evaluation (tools/test_supernet.py), not training.
    ``fp16`` is that key's value: with the fp16 hook, ``fp16 = dict(attention=True)`` makes the hook wrap
    the model for fp16 attention as well; without the hook it changes nothing
    here.  Its type is checked either way."""
    from ..core.fp16_utils import check_fp16_cfg
    attention = check_fp16_cfg(fp16)
    oc = dict(optimizer_config or {})
    if oc.get("grad_clip"):
        raise NotImplementedError("grad_clip")
    if oc.pop("type", None) == "Fp16OptimizerHook":
        return Fp16ArenaOptimizerHook(attention=attention, **oc)
    return ArenaOptimizerHook()


def check_lr_policy(cfg):
    """``cfg.lr_config`` -> (policy, its other keys); anything but 'poly' and 'fixed' is refused."""
    lrc = dict(cfg.get("lr_config") or dict(policy="fixed"))
    policy = lrc.pop("policy", "fixed")
    if policy not in ("poly", "fixed"):
        raise NotImplementedError("lr_config.policy=%r: only 'poly' and 'fixed'" % (policy,))
    return policy, lrc


def check_input_shape_cfg(cfg):
    """``apply_input_shape`` (elastic input resolution): the flag's value, after
    refusing what it does not combine with (in-place distillation: teacher and students at different
    resolutions are out of scope)."""
    apply = bool(cfg.get("apply_input_shape", False))
    if apply and cfg.get("use_distillation", False):
        raise ValueError(SANDWICH_INPUT_SHAPE)
    return apply


def prepare_training(model, cfg):
    """The part of a training set-up that belongs to the MODEL, not to a run: the model on the
    device, its parameter arena (after the DDP wrap-time broadcast, gaiaseg/apis/train.py:88-96), the
    gradient reducer over it and the parameter groups of ``cfg.optimizer``.  train_segmentor makes
    one per call; apis/finetune.py makes one for a whole model space."""
    device = torch.device("cuda", torch.cuda.current_device())
    model = model.to(device)
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)   # the DDP wrap-time broadcast (:88-96)
    reducer = gdist.GradReducer(arena.flat_grad, arena.segments,
                                bucket_bytes=cfg.get("bucket_bytes", 64 << 20))
    # optimizer keys the arena SGD does not implement are errors, and paramwise_cfg becomes parameter
    # groups (core/optimizer.py; None = the one-group path)
    opt = check_optimizer_cfg(cfg.optimizer)
    if opt.get("type", "SGD") == "AdamW":    # second moment + per-parameter counters, per-parameter tables
        arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    param_groups = build_param_groups(model, cfg.optimizer)
    return model, arena, reducer, param_groups


def run_training(model, arena, reducer, param_groups, train_sampler, val_sampler, dataset, cfg,
                 opt_hook, validate=False, meta=None, logger=None, val_loader=None,
                 eval_num_batches=None, checkpoints=True, before_run=None):
    """The body of train_segmentor on a prepared (model, arena, reducer, parameter groups): build the
    runner, register the hooks ``cfg`` names, load ``cfg.resume_from`` / ``cfg.load_from``, apply
    ``caliberate_bn.reset_stats``, build the train loader and run.  ``dataset`` is a dataset config
    or an iterable of batches (a loader built earlier passes through build_dataloader untouched).
    ``val_loader`` / ``eval_num_batches``: a prepared loader and batch count for the CrossArchEvalHook
    instead of the ones ``cfg`` describes.  ``checkpoints=False`` registers no CheckpointHook and
    reads no checkpoint (the caller owns the weights).  ``before_run(runner)`` is called right before
    ``runner.run``."""
    device = arena.device
    apply_input_shape = check_input_shape_cfg(cfg)
    opt = check_optimizer_cfg(cfg.optimizer)      # (AdamW: torch's defaults filled in)
    lr = opt["lr"]
    lr_scaler = cfg.get("lr_scaler")      # gaiaseg/apis/train.py:103-113
    if lr_scaler is not None:
        total_batch = cfg.data["samples_per_gpu"] * gdist.world_size()
        if lr_scaler.get("policy", "linear") == "linear":
            lr = lr_scaler["base_lr"] * total_batch
        else:
            lr = lr_scaler["base_lr"] * total_batch ** lr_scaler.get("temperature", 0.5)
    runner = IterBasedRunner(model, arena, reducer, base_lr=lr, momentum=opt.get("momentum", 0.0),
                             weight_decay=opt.get("weight_decay", 0.0),
                             max_iters=cfg.runner["max_iters"], work_dir=cfg.get("work_dir"),
                             logger=logger, meta=meta, param_groups=param_groups,
                             apply_input_shape=apply_input_shape)
    if cfg.get("use_distillation", False):
        # the sandwich iteration takes the place of the one-subnet draw (core/runner.py SandwichHook);
        # train_sampler is the concat of sandwich_train_sampler(cfg)
        check_sandwich_model(model)
        runner.register_hook(SandwichHook(train_sampler, cfg.get("distill_cfg")))
    elif cfg.get("manipulate_arch", True):  # :142-146
        runner.register_hook(ManipulateArchHook(train_sampler))
    policy, lrc = check_lr_policy(cfg)
    runner.register_hook(PolyLrUpdaterHook(**lrc) if policy == "poly" else FixedLrUpdaterHook(**lrc))
    runner.register_hook(opt_hook)
    ck = cfg.get("checkpoint_config")
    if ck and checkpoints:
        runner.register_hook(CheckpointHook(**dict(ck)))
    lg = cfg.get("log_config")
    if lg:
        runner.register_hook(TextLoggerHook(interval=lg.get("interval", 50), logger=logger))
    if validate and cfg.get("evaluation"):
        # gaiaseg/apis/train.py:150-170: (Dist)CrossArchEvalHook over the val anchors
        from ..core.evaluation import CrossArchEvalHook
        ev = dict(cfg.evaluation)
        if val_loader is None:
            val_cfg = cfg.data.get("val") or cfg.data["train"]
            val_loader = build_dataloader(val_cfg, cfg.data["samples_per_gpu"], seed=12345,
                                          device=device, train=cfg.data.get("val") is None,
                                          workers_per_gpu=cfg.data.get("workers_per_gpu", 2),
                                          device_cache_gb=cfg.data.get("device_cache_gb"))
        # ``caliberate_bn.recalibrate``: the anchors are scored under re-calibrated BatchNorm statistics
        from ..core.bn_calibration import BNCalibrator, build_calibration_batches
        calib = build_calibration_batches(cfg, device=device, num_classes=model.num_classes)
        runner.register_hook(CrossArchEvalHook(val_loader, val_sampler,
                                               interval=ev.get("interval", 8000),
                                               num_batches=eval_num_batches or ev.get("num_batches", 4),
                                               num_classes=model.num_classes, logger=logger,
                                               apply_input_shape=apply_input_shape,
                                               calibrator=BNCalibrator(model, calib)
                                               if calib is not None else None))
    if checkpoints:
        if cfg.get("resume_from"):
            runner.resume(cfg.resume_from)
        elif cfg.get("load_from"):
            runner.load_checkpoint(cfg.load_from)
    from .test import apply_bn_calibration
    apply_bn_calibration(model, cfg.get("caliberate_bn"), "train")   # gaiaseg/apis/train.py:177-184
    loader = build_dataloader(dataset, cfg.data["samples_per_gpu"], seed=cfg.get("seed") or 0,
                              device=device, workers_per_gpu=cfg.data.get("workers_per_gpu", 2),
                              device_cache_gb=cfg.data.get("device_cache_gb"))
    if before_run is not None:
        before_run(runner)
    runner.run([loader], cfg.get("workflow", [("train", 1)]))
    return runner


def train_segmentor(model, train_sampler, val_sampler, dataset, cfg, distributed=False,
                    validate=False, timestamp=None, meta=None, logger=None):
    opt_hook = optimizer_hook(cfg.get("optimizer_config"), cfg.get("fp16"))
    check_input_shape_cfg(cfg)
    if cfg.get("use_distillation", False) and isinstance(opt_hook, Fp16ArenaOptimizerHook):
        raise ValueError("use_distillation with fp16 training (optimizer_config type "
                         "'Fp16OptimizerHook') is not supported")
    model, arena, reducer, param_groups = prepare_training(model, cfg)
    return run_training(model, arena, reducer, param_groups, train_sampler, val_sampler, dataset, cfg,
                        opt_hook, validate=validate, meta=meta, logger=logger)
