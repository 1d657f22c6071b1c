#!/usr/bin/env python
"""Fast-finetune the best subnets of a model space — the interface of the reference's
tools/finetune_supernet.py (:44-136): load a supernet checkpoint ONCE, select subnets from a
model-space file with ``model_sampling_rules`` (typically the top rows by ``metric.direct.mIoU`` of
tools/test_supernet.py's output), train each one for ``runner.max_iters`` iterations from the
supernet's weights as a one-anchor run, evaluate it, and write the input rows plus
``metric.<tag>.*`` to ``<work-dir>/finetune_supernet/<out-name>``, a model-space file the next rule
can rank (``dict(type='sample', operation='top', key='metric.finetune.mIoU', value=1)``).

    python tools/finetune_supernet.py CONFIG --load-from CKPT --model-space-path metrics.json --work-dir W
    python -m torch.distributed.run --nproc-per-node 8 tools/finetune_supernet.py ... --launcher pytorch

The supernet stays on the device for the whole model space: every subnet starts from a device-side
snapshot of it (gaia_seg_amd/apis/finetune.py), so a row does not depend on
which other subnets were finetuned before it.  ``optimizer.lr=0`` gives a calibration-only run (the
BatchNorm running statistics of each subnet re-estimated on the train data, no weight moves).

Deviations from the reference:
  * its hard-coded list of skipped ``overhead.flops`` values (:266) is not reproduced;
  * ``data.input_shape`` is carried through the rows; with ``cfg.apply_input_shape = True`` each
    row is trained and evaluated at its own input size and rows of one arch at different sizes are
    rows of their own (the reference has that code commented out, :275-277);
  * step and by-epoch ``lr_config`` schedules (the reference's detection finetune configs) stay
    refused: 'poly' and 'fixed' by iteration only;
  * the output file is rewritten (atomically) after EVERY subnet, and two flags are added where the
    reference has ``TODO: add checkpointing`` (:360): ``--resume`` skips the subnets whose arch
    already carries this metric tag in the existing output file, ``--keep-checkpoints`` saves every
    finetuned subnet in the supernet's checkpoint format (tools/extract_subnet.py cuts it out);
  * ``--gpus`` / ``--gpu-ids`` / ``--tmpdir`` / ``--gpu-collect`` are accepted without effect:
    nothing is gathered through the file system (one all-reduce of a confusion matrix per subnet).
"""
import argparse
import hashlib
import json
import logging
import os
import os.path as osp
import re
import sys
import time

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gaia_seg_amd import __version__  # noqa: E402
from gaia_seg_amd.apis import finetune_model_space, set_random_seed  # noqa: E402
from gaia_seg_amd.apis.finetune import check_finetune_cfg  # noqa: E402
from gaia_seg_amd.apis.train import build_dataloader  # noqa: E402
from gaia_seg_amd.core.checkpoint import load_checkpoint, save_checkpoint  # noqa: E402
from gaia_seg_amd.core.config import Config, DictAction  # noqa: E402
from gaia_seg_amd.core.model_space import (ModelSpace, _listify, arch_key,  # noqa: E402
                                           dump_model_space, load_model_space)
from gaia_seg_amd.models import build_segmentor  # noqa: E402

# options of the reference's CLI that this tool does not implement: (flag, reason)
UNSUPPORTED = [
    ("save_results", "--save-results: per-image result dumps are not supported"),
    ("out", "--out: per-image result files are not supported (the rows go to "
            "<work-dir>/finetune_supernet/<out-name>)"),
]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Fast-finetune the subnets of a model space")
    parser.add_argument("config", help="finetune config file path")
    parser.add_argument("--work-dir", help="output goes to <work-dir>/finetune_supernet/<out-name>")
    parser.add_argument("--no-validate", action="store_true",
                        help="whether not to evaluate the subnet during its training")
    parser.add_argument("--load-from", help="supernet checkpoint (else cfg.load_from)")
    parser.add_argument("--model-space-path", dest="model_space_path", default=None,
                        help="model-space file (JSON list or JSON lines; else cfg.model_space_path)")
    parser.add_argument("--tmpdir", help="accepted without effect")
    parser.add_argument("--metric-tag", default="finetune",
                        help="columns are written as metric.<tag>.mIoU / mAcc / aAcc")
    parser.add_argument("--out", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--out-name", default="metrics.json", help="output file name")
    parser.add_argument("--save-results", action="store_true", help=argparse.SUPPRESS)
    parser.add_argument("--gpu-collect", action="store_true", help="accepted without effect")
    parser.add_argument("--eval", nargs="+", default=["mIoU"], help="metrics (mIoU only)")
    parser.add_argument("--eval-options", nargs="+", default=None,
                        help="custom options for evaluation (none are supported)")
    group_gpus = parser.add_mutually_exclusive_group()
    group_gpus.add_argument("--gpus", type=int, help="accepted without effect")
    group_gpus.add_argument("--gpu-ids", type=int, nargs="+", help="accepted without effect")
    parser.add_argument("--seed", type=int, default=None, help="random seed (every subnet starts from it)")
    parser.add_argument("--deterministic", action="store_true")
    parser.add_argument("--options", nargs="+", default=None,
                        help="custom options (deprecated: --cfg-options)")
    parser.add_argument("--cfg-options", nargs="+", default=None,
                        help="override settings in the config, key=value pairs")
    parser.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="none")
    parser.add_argument("--local_rank", "--local-rank", type=int, default=0)
    parser.add_argument("--resume", action="store_true",
                        help="skip the subnets that already carry this metric tag in the output file")
    parser.add_argument("--keep-checkpoints", action="store_true",
                        help="save every finetuned subnet to <work-dir>/finetune_supernet/ckpt/<name>.pth")
    args = parser.parse_args(argv)
    for flag, why in UNSUPPORTED:
        if getattr(args, flag):
            parser.error(why)
    if args.launcher in ("slurm", "mpi"):
        parser.error("--launcher %s is not supported: use --launcher pytorch under "
                     "torch.distributed.run" % args.launcher)
    if args.options and args.cfg_options:
        parser.error("--options and --cfg-options cannot be both specified, --options is deprecated "
                     "in favor of --cfg-options")
    bad = [m for m in args.eval if m != "mIoU"]
    if bad:
        parser.error("--eval: only mIoU is supported, got %s" % " ".join(bad))
    if args.eval_options:
        parser.error("--eval-options: no evaluation options are supported (got %s)"
                     % " ".join(args.eval_options))
    if "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = str(args.local_rank)
    return args


def select_metas(cfg, model_space_path):
    """The rows of the model space that ``cfg.model_sampling_rules`` select, in the rules' order."""
    ms = ModelSpace.load(model_space_path)
    rules = cfg.get("model_sampling_rules")
    if rules:
        ms = ms.apply_rule(rules)
    return ms.rows


def has_tag(row, tag):
    return all("metric.%s.%s" % (tag, k) in row for k in ("mIoU", "mAcc", "aAcc"))


def scale_key(meta):
    """A row's identity with ``cfg.apply_input_shape``: its arch and its input size."""
    v = meta.get("data.input_shape")
    return arch_key(meta), tuple(v) if isinstance(v, (list, tuple)) else v


def pending_metas(metas, existing_rows, tag, key=arch_key):
    """``--resume``: the metas whose arch has no ``metric.<tag>.*`` in the existing output rows."""
    done = {key(r) for r in existing_rows if has_tag(r, tag)}
    return [m for m in metas if key(m) not in done]


def merge_rows(metas, existing_rows, new_rows, tag, key=arch_key):
    """The output file's rows: one per selected meta in selection order -- the freshly finetuned row,
    else the existing row that carries the tag -- then the existing rows outside the selection."""
    new = {key(r): r for r in new_rows}
    old = {key(r): r for r in existing_rows if has_tag(r, tag)}
    out, used = [], set()
    for m in metas:
        k = key(m)
        r = new.get(k) or old.get(k)
        if r is not None and k not in used:
            out.append(r)
            used.add(k)
    out.extend(r for r in existing_rows if key(r) not in used)
    return out


def write_rows(rows, path):
    """Atomically: a reader (or a later --resume) sees the old file or the new one, never a torn one."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    dump_model_space(rows, tmp)
    os.replace(tmp, path)


def checkpoint_name(row):
    """The row's name, made safe for a file name; a row without one is named by the md5 of its arch
    (as tools/extract_subnet.py names its files)."""
    if row.get("name") is not None:
        return re.sub(r"[^A-Za-z0-9_.+-]", "_", str(row["name"]))
    arch = {k: v for k, v in _listify(dict(row)).items() if k.startswith("arch")}
    return hashlib.md5(json.dumps(arch, sort_keys=True).encode()).hexdigest()[:8]


def get_logger(log_file=None, log_level="INFO"):
    logger = logging.getLogger("gaia_seg_amd")
    if not logger.handlers:
        rank = dist.get_rank() if dist.is_initialized() else 0
        handlers = [logging.StreamHandler()]
        if rank == 0 and log_file is not None:
            handlers.append(logging.FileHandler(log_file, "w"))
        fmt = logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s")
        for h in handlers:
            h.setFormatter(fmt)
            logger.addHandler(h)
        logger.setLevel(log_level if rank == 0 else logging.ERROR)
    return logger


def main(argv=None):
    args = parse_args(argv)
    cfg = Config.fromfile(args.config)
    options = DictAction.parse(args.cfg_options or args.options)
    if options:
        cfg.merge_from_dict(options)
    if args.work_dir is not None:
        cfg.work_dir = args.work_dir
    elif cfg.get("work_dir", None) is None:
        cfg.work_dir = osp.join("./work_dirs", osp.splitext(osp.basename(args.config))[0])
    if args.load_from is not None:
        cfg.load_from = args.load_from
    if not cfg.get("load_from"):
        raise SystemExit("finetune_supernet: a supernet checkpoint is required (--load-from or cfg.load_from)")
    if not osp.exists(cfg.load_from):
        raise SystemExit("finetune_supernet: `%s` not existed." % cfg.load_from)
    space_path = args.model_space_path if args.model_space_path not in (None, "None") \
        else cfg.get("model_space_path")
    if not space_path:
        raise SystemExit("finetune_supernet: a model space is required (--model-space-path or "
                         "cfg.model_space_path)")
    if args.launcher == "none":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    else:
        local_rank = int(os.environ["LOCAL_RANK"])
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = dict(cfg.get("dist_params") or dict(backend="nccl")).get("backend", "nccl")
        dist.init_process_group(backend=backend, device_id=torch.device("cuda", local_rank))
    rank = dist.get_rank() if dist.is_initialized() else 0

    out_dir = osp.join(cfg.work_dir, "finetune_supernet")
    os.makedirs(out_dir, exist_ok=True)
    out = osp.join(out_dir, args.out_name)
    timestamp = time.strftime("%Y%m%d_%H%M%S", time.localtime())
    logger = get_logger(osp.join(cfg.work_dir, "%s.log" % timestamp), cfg.get("log_level", "INFO"))
    seed = args.seed if args.seed is not None else 0
    logger.info("Set random seed to %s for every subnet, deterministic: %s" % (seed, args.deterministic))
    set_random_seed(seed, deterministic=args.deterministic)
    cfg.seed = args.seed

    metas = select_metas(cfg, space_path)
    logger.info("Model space file loaded: %s (%d subnets selected)" % (space_path, len(metas)))
    if not metas:
        raise SystemExit("finetune_supernet: the sampling rules selected no subnet")
    if not any(k.startswith("metric.") for m in metas for k in m):
        logger.warning("`metric` is absent during finetuning.")
    existing = load_model_space(out) if args.resume and osp.exists(out) else []
    key = scale_key if cfg.get("apply_input_shape", False) else arch_key
    todo = pending_metas(metas, existing, args.metric_tag, key)
    if len(todo) < len(metas):
        logger.info("--resume: %d of %d subnets already carry metric.%s in %s"
                    % (len(metas) - len(todo), len(metas), args.metric_tag, out))
    if not todo:
        logger.info("nothing left to finetune")
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    check_finetune_cfg(cfg, todo)

    val_cfg = cfg.data.get("val")
    synthetic = val_cfg is None or dict(val_cfg).get("type") == "SyntheticSegDataset"
    ev = dict(cfg.get("evaluation") or {})
    num_batches = ev.get("num_batches")
    if synthetic and not num_batches:
        raise SystemExit("finetune_supernet: a synthetic val set needs evaluation.num_batches "
                         "(--cfg-options evaluation.num_batches=N)")
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    ck = load_checkpoint(model, cfg.load_from, strict=False, logger=logger)   # the ONLY checkpoint read
    model = model.cuda()
    val_loader = build_dataloader(val_cfg or cfg.data["train"], cfg.data.get("samples_per_gpu", 1),
                                  seed=12345, device="cuda", num_classes=model.num_classes,
                                  train=synthetic, workers_per_gpu=cfg.data.get("workers_per_gpu", 2),
                                  device_cache_gb=cfg.data.get("device_cache_gb"))
    if synthetic:
        # the synthetic loader cycles a pool of batches without restarting: every subnet must see
        # the same batches
        it = iter(val_loader)
        val_loader = [next(it) for _ in range(num_batches)]
    elif not num_batches:
        num_batches = len(val_loader)   # one pass over this rank's shard per subnet

    done = []
    ck_meta = {k: v for k, v in ck.get("meta", {}).items() if k not in ("iter", "fp16")}

    def on_subnet(row, net):
        done.append(row)
        if args.keep_checkpoints:
            # every rank reads its state (collective-free), rank 0 writes
            path = osp.join(out_dir, "ckpt", "%s.pth" % checkpoint_name(row))
            if rank == 0:
                save_checkpoint(net, path, meta=dict(ck_meta, version=__version__, **_listify(dict(row))))
        if rank == 0:
            write_rows(merge_rows(metas, existing, done, args.metric_tag, key), out)

    rows = finetune_model_space(model, todo, cfg, cfg.data["train"], val_loader, num_batches,
                                metric_tag=args.metric_tag, validate=not args.no_validate, seed=seed,
                                logger=logger, on_subnet=on_subnet)
    if rank == 0:
        for r in rows:
            print("%s mIoU %.4f mAcc %.4f aAcc %.4f" % (
                r.get("name", "-"), r["metric.%s.mIoU" % args.metric_tag],
                r["metric.%s.mAcc" % args.metric_tag], r["metric.%s.aAcc" % args.metric_tag]))
        print("wrote %d rows to %s" % (len(merge_rows(metas, existing, done, args.metric_tag, key)), out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
