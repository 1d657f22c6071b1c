#!/usr/bin/env python
"""Rank the subnets of a model space on the validation set — the interface of the reference's
tools/test_supernet.py: load a supernet checkpoint, select subnets from a model-space file with
``model_sampling_rules``, evaluate each one, and write the input rows plus ``metric.<tag>.*`` to
``<work-dir>/test_supernet/<out-name>``, a model-space file the next round of rules can rank
(``dict(type='sample', operation='top', key='metric.direct.mIoU', value=1)``).

    python tools/test_supernet.py CONFIG CHECKPOINT --model-space-path flops.json --work-dir W
    python -m torch.distributed.run --nproc-per-node 8 tools/test_supernet.py ... --launcher pytorch

Without a model-space path (option or ``cfg.model_space_path``) the val sampler's ``traverse()``
supplies the metas.  ``cfg.fp16`` runs the convolutions on fp16 operands (wrap_fp16_model).
``cfg.caliberate_bn.use_minibatch_stats`` normalises with the statistics of each batch.  A
synthetic val set (no ``data.val``) needs ``evaluation.num_batches``; a file-backed one is read
once per subnet unless ``evaluation.num_batches`` says otherwise.  ``data.input_shape`` is carried
through the rows but not applied (the reference's scale manipulation is commented out as well).
"""
import argparse
import os
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gaia_seg_amd.apis import set_random_seed  # noqa: E402
from gaia_seg_amd.apis.test import test_model_space  # noqa: E402
from gaia_seg_amd.apis.train import build_dataloader  # noqa: E402
from gaia_seg_amd.core.checkpoint import load_checkpoint  # noqa: E402
from gaia_seg_amd.core.config import Config, DictAction  # noqa: E402
from gaia_seg_amd.core.fp16_utils import wrap_fp16_model  # noqa: E402
from gaia_seg_amd.core.model_space import (ModelSpace, build_model_sampler,  # noqa: E402
                                           dump_model_space)
from gaia_seg_amd.models import build_segmentor  # noqa: E402

# options of the reference's CLI that this tool does not implement: (flag, reason)
UNSUPPORTED = [
    ("show", "--show: visualisation is not supported"),
    ("show_dir", "--show-dir: visualisation is not supported"),
    ("format_only", "--format-only: per-image result files are not supported"),
    ("save_results", "--save-results: per-image result dumps are not supported"),
    ("aug_test", "--aug-test is not supported: the val loader has no multi-scale / flip pipeline"),
]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate the subnets of a model space")
    parser.add_argument("config", help="test config file path")
    parser.add_argument("checkpoint", help="supernet checkpoint file")
    parser.add_argument("--model-space-path", help="model-space file (JSON list or JSON lines)")
    parser.add_argument("--work-dir", help="output goes to <work-dir>/test_supernet/<out-name>")
    parser.add_argument("--out-name", default="metrics.json", help="output file name")
    parser.add_argument("--eval", nargs="+", default=["mIoU"], help="metrics (mIoU only)")
    parser.add_argument("--aug-test", action="store_true", help="use flip and multi-scale test")
    parser.add_argument("--metric-tag", default="direct",
                        help="columns are written as metric.<tag>.mIoU / mAcc / aAcc")
    parser.add_argument("--options", nargs="+", default=None,
                        help="custom options (deprecated: --cfg-options)")
    parser.add_argument("--cfg-options", nargs="+", default=None,
                        help="override settings in the config, key=value pairs")
    parser.add_argument("--eval-options", nargs="+", default=None,
                        help="custom options for evaluation (none are supported)")
    parser.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="none")
    parser.add_argument("--local_rank", "--local-rank", type=int, default=0)
    parser.add_argument("--seed", type=int, default=None, help="random seed")
    parser.add_argument("--show", action="store_true", help=argparse.SUPPRESS)
    parser.add_argument("--show-dir", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--format-only", action="store_true", help=argparse.SUPPRESS)
    parser.add_argument("--save-results", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args(argv)
    for flag, why in UNSUPPORTED:
        if getattr(args, flag):
            parser.error(why)
    if args.launcher in ("slurm", "mpi"):
        parser.error("--launcher %s is not supported: use --launcher pytorch under "
                     "torch.distributed.run" % args.launcher)
    bad = [m for m in args.eval if m != "mIoU"]
    if bad:
        parser.error("--eval: only mIoU is supported, got %s" % " ".join(bad))
    if args.eval_options:
        parser.error("--eval-options: no evaluation options are supported (got %s)"
                     % " ".join(args.eval_options))
    if "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = str(args.local_rank)
    return args


def select_metas(cfg, args):
    """The model space and its rules, or the val sampler's subnets."""
    path = args.model_space_path or cfg.get("model_space_path")
    if path:
        ms = ModelSpace.load(path)
        rules = cfg.get("model_sampling_rules")
        if rules:
            ms = ms.apply_rule(rules)
        return ms.rows
    sampler = build_model_sampler(cfg.val_sampler)
    sampler.set_mode("traverse")
    return sampler.traverse()


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
    if args.launcher == "none":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    else:
        local_rank = int(os.environ["LOCAL_RANK"])
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = dict(cfg.get("dist_params") or dict(backend="nccl")).get("backend", "nccl")
        dist.init_process_group(backend=backend, device_id=torch.device("cuda", local_rank))
    if args.seed is not None:
        set_random_seed(args.seed)

    metas = select_metas(cfg, args)
    if not metas:
        raise SystemExit("test_supernet: the sampling rules selected no subnet")
    val_cfg = cfg.data.get("val")
    synthetic = val_cfg is None or dict(val_cfg).get("type") == "SyntheticSegDataset"
    ev = dict(cfg.get("evaluation") or {})
    num_batches = ev.get("num_batches")
    if synthetic and not num_batches:
        raise SystemExit("test_supernet: a synthetic val set needs evaluation.num_batches "
                         "(--cfg-options evaluation.num_batches=N)")
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    load_checkpoint(model, args.checkpoint, strict=False)
    model = model.cuda().eval()
    if cfg.get("fp16", None) is not None:
        wrap_fp16_model(model)
    loader = build_dataloader(val_cfg or cfg.data["train"], cfg.data.get("samples_per_gpu", 1),
                              seed=12345, device="cuda", num_classes=model.num_classes,
                              train=synthetic,
                              workers_per_gpu=cfg.data.get("workers_per_gpu", 2),
                              device_cache_gb=cfg.data.get("device_cache_gb"))
    if synthetic:
        # the synthetic loader cycles a pool of batches without restarting: every subnet must see
        # the same batches
        it = iter(loader)
        loader = [next(it) for _ in range(num_batches)]
    elif not num_batches:
        num_batches = len(loader)   # one pass over this rank's shard per subnet
    rows = test_model_space(model, loader, metas, num_batches, model.num_classes,
                            calib_cfg=cfg.get("caliberate_bn"), metric_tag=args.metric_tag)
    rank = dist.get_rank() if dist.is_initialized() else 0
    if rank == 0:
        out_dir = osp.join(cfg.work_dir, "test_supernet")
        os.makedirs(out_dir, exist_ok=True)
        out = osp.join(out_dir, args.out_name)
        dump_model_space(rows, out)
        for r in rows:
            print("%s mIoU %.4f mAcc %.4f aAcc %.4f" % (
                r.get("name", "-"), r["metric.%s.mIoU" % args.metric_tag],
                r["metric.%s.mAcc" % args.metric_tag], r["metric.%s.aAcc" % args.metric_tag]))
        print("wrote %d rows to %s" % (len(rows), out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
