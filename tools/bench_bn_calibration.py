#!/usr/bin/env python
"""Per-subnet BatchNorm re-calibration (core/bn_calibration.py, gs_bn_calib_fold) measured on the FCN
supernet (configs/supernet/fcn_ar50to101v2.py) at 1024x512, bs 2:

    python tools/bench_bn_calibration.py [--anchors MIN,R50,MAX] [--batches 32] [--rounds 5]
                                         [--reps 50] [--no-finetune] [--md out.md]

Per anchor, warmed, the median of --rounds rounds (min..max next to it):
(a) one subnet's calibration: host wall time, device synchronised, of an empty
    ``with calibrator.calibrated(): pass`` over --batches resident batches (layer table cached, as for
    the second visit of a subnet), and its parts: the K forwards, the K fold launches + the commit
    (K + 1 launches of gs_bn_calib_fold, device events), the save and the restore (2 launches);
(b) the same batches through the route that existed before: --batches training iterations with lr 0
    (forward + backward + SGD on a runner; what tools/finetune_supernet.py with optimizer.lr=0 does
    per subnet, without its snapshot restore);
(c) the fold launch alone (ADD) against the same accumulation written as tensor operations: per layer
    two slices and two in-place adds, 4 x n_layers operations.
bench.py (the training headline) is not involved: no training code path reads this module."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

N, H, W = 2, 512, 1024


def anchor_meta(cfg, name):
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:
        if m.get("name") == name:
            return dict(m)
    raise KeyError(name)


def make_batches(k):
    g = torch.Generator().manual_seed(0)
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False) for _ in range(N)]
    return [dict(img=torch.randn(N, 3, H, W, generator=g).cuda(), img_metas=metas,
                 gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda()) for _ in range(k)]


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3       # ms


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


def _med(xs):
    return statistics.median(xs), min(xs), max(xs)


def bench_anchor(args, cfg, model, runner, name, batches):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.dynamic import fold_dict
    meta = anchor_meta(cfg, name)
    model.eval()
    model.manipulate_arch(fold_dict(meta)["arch"])
    cal = BNCalibrator(model, batches)

    def whole():
        with cal.calibrated():
            pass

    def forwards():
        for b in batches:
            cal._forward(b["img"])

    whole()                                         # builds the layer table, warms the plans
    t = cal._table(batches[0]["img"])
    total = [_wall(whole) for _ in range(args.rounds)]
    # the K forwards alone, in the state the calibration runs them in (batch statistics, momentum 1)
    model.eval()
    cal._fold(t, t.save, lib.BN_CALIB_SAVE)
    found = [(m, m.momentum) for m in t.mods]
    for m in t.mods:
        m.training, m.momentum = True, 1.0
        m.__dict__.pop("_bnp_cache", None)
    forwards()
    fwd = [_wall(forwards) for _ in range(args.rounds)]
    for m, momentum in found:
        m.training, m.momentum = False, momentum
        m.__dict__.pop("_bnp_cache", None)
        m.__dict__["_nbt_pending"] = 0
    cal._fold(t, t.save, lib.BN_CALIB_WRITE, 1.0)

    # (c) the fold launch against tensor operations; the running buffers are only read
    def fold():
        cal._fold(t, t.acc, lib.BN_CALIB_ADD)
    am = [torch.zeros(c, device="cuda") for c in t.widths]
    av = [torch.zeros(c, device="cuda") for c in t.widths]

    def tensor_ops():
        for m, c, a, v in zip(t.mods, t.widths, am, av):
            a.add_(m.running_mean[:c])
            v.add_(m.running_var[:c])
    for fn in (fold, tensor_ops):
        _events(fn, 3)
    tf, tt = [], []
    for _ in range(args.rounds):
        tf.append(_events(fold, args.reps))
        tt.append(_events(tensor_ops, args.reps))
    tw = [_wall(tensor_ops) * 1e3 for _ in range(args.rounds)]    # host-bound: wall time per pass, us

    # (b) lr = 0 training iterations over the same batches
    ft = None
    if runner is not None:
        model.train()
        runner.set_arch(meta)

        def train():
            for b in batches:
                runner.train_iter(b)
        train()
        ft = [_wall(train) for _ in range(args.rounds)]
        model.eval()
    k = len(batches)
    fold_us = statistics.median(tf)
    row = dict(name=name, layers=t.n, floats=t.floats, total=_med(total), fwd=_med(fwd),
               folds_ms=(k + 1) * fold_us / 1e3, save_restore_ms=2 * fold_us / 1e3, fold=_med(tf),
               tensor=_med(tt), tensor_wall=_med(tw), finetune=_med(ft) if ft else None)
    print("%-4s %3d layers %6d floats | calibration %8.2f ms (%.2f..%.2f) = forwards %8.2f ms (%.2f..%.2f) + "
          "%d folds %.3f ms + save/restore %.3f ms | fold %.1f us (%.1f..%.1f) vs %d tensor ops %.1f us "
          "(%.1f..%.1f) on the device, %.1f us (%.1f..%.1f) wall"
          % ((name, t.n, t.floats) + row["total"] + row["fwd"] + (k + 1, row["folds_ms"], row["save_restore_ms"])
             + row["fold"] + (4 * t.n,) + row["tensor"] + row["tensor_wall"]), flush=True)
    if ft:
        print("     lr=0 training route: %8.2f ms (%.2f..%.2f), x%.2f of the calibration"
              % (row["finetune"] + (row["finetune"][0] / row["total"][0],)), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", default="MIN,R50,MAX")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-finetune", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_calibration.py measures on the MI355X: no GPU found")
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = None
    if not args.no_finetune:
        opt = dict(cfg.optimizer)
        runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.0,
                                 momentum=opt["momentum"], weight_decay=opt["weight_decay"], max_iters=10 ** 6)
        runner.register_hook(FixedLrUpdaterHook())
        runner.register_hook(ArenaOptimizerHook())
        runner.call_hook("before_run")
    batches = make_batches(args.batches)
    rows = [bench_anchor(args, cfg, model, runner, a, batches) for a in args.anchors.split(",") if a]
    if args.md:
        with open(args.md, "w") as f:
            f.write("| subnet | BN layers | bank floats | calibration ms (min..max) | forwards ms (min..max) | "
                    "%d folds ms | save + restore ms | lr=0 training ms (min..max) | ratio |\n"
                    "|---|---|---|---|---|---|---|---|---|\n" % (args.batches + 1))
            for r in rows:
                ft = r["finetune"]
                f.write("| %s | %d | %d | %.2f (%.2f..%.2f) | %.2f (%.2f..%.2f) | %.3f | %.3f | %s | %s |\n"
                        % ((r["name"], r["layers"], r["floats"]) + r["total"] + r["fwd"]
                           + (r["folds_ms"], r["save_restore_ms"],
                              "%.2f (%.2f..%.2f)" % ft if ft else "-",
                              "%.2f" % (ft[0] / r["total"][0]) if ft else "-")))
            f.write("\n| subnet | gs_bn_calib_fold us (min..max) | tensor ops | device us (min..max) | "
                    "wall us (min..max) | device ratio | wall ratio |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %.1f (%.1f..%.1f) | %d | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.1f | %.1f |\n"
                        % ((r["name"],) + r["fold"] + (4 * r["layers"],) + r["tensor"] + r["tensor_wall"]
                           + (r["tensor"][0] / r["fold"][0], r["tensor_wall"][0] / r["fold"][0])))


if __name__ == "__main__":
    main()
