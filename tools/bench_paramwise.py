#!/usr/bin/env python
"""The table-driven grouped SGD (gs_sgd_step_groups, paramwise_cfg) measured on the FCN supernet
(configs/supernet/fcn_ar50to101v2_paramwise.py):

    python tools/bench_paramwise.py [--anchors MAX,R50,MIN] [--chunks 4096,16384,65536] [--rounds 5]
                                    [--reps 20] [--steps 10] [--passes 5] [--no-kernel] [--no-steps]
                                    [--md out.md]

(a) kernel alone, device events, warmed: per anchor and chunk size CH, one gs_sgd_step_groups launch
    over the subnet's chunk table against gs_sgd_step over the same merged ranges (one launch per
    range), alternating in one process, --rounds rounds of --reps repetitions each; median and the
    min..max spread of the rounds.  Bytes moved = 24 B per element (read p, g, m; write p, m, g);
    the share is of the 8.0 TB/s HBM3E peak (6.29 TB/s is what a float4 copy reaches).
(b) training images/s (1024x512 crops, bs 2) of the paramwise config against the same config without
    paramwise_cfg, two runners in one process, passes alternating, median of --passes.
bench.py (the training headline) is not involved."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

HBM_PEAK = 8.0e12
N, H, W = 2, 512, 1024


def anchor_meta(cfg, name):
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:
        if m.get("name") == name:
            return dict(m)
    raise KeyError(name)


def make_runner(cfg, grouped):
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, PolyLrUpdaterHook
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    opt = dict(cfg.optimizer)
    if not grouped:
        opt.pop("paramwise_cfg", None)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=opt["momentum"], weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             param_groups=build_param_groups(model, opt))
    lrc = dict(cfg.lr_config)
    lrc.pop("policy")
    runner.register_hook(PolyLrUpdaterHook(**lrc))
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per optimizer step


def bench_kernel(args, cfg, runner):
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    L = lib.load()
    arena, pg = runner.arena, runner.param_groups
    st = current_stream_ptr()
    pb, gb, mb = arena.flat_param.data_ptr(), arena.flat_grad.data_ptr(), arena.flat_mom.data_ptr()
    lr, wd = 1e-6, 5e-4
    arena.write_group_hyper([lr] * len(pg), [wd] * len(pg), 0.9, 1.0)
    rows = []
    for name in [a for a in args.anchors.split(",") if a]:
        runner.set_arch(anchor_meta(cfg, name))
        ranges = list(runner.active_ranges)
        elems = sum(b - a for a, b in ranges)

        def base():
            for a, b in ranges:
                L.gs_sgd_step(pb + 4 * a, gb + 4 * a, mb + 4 * a, b - a, lr, 0.9, wd, 1.0, 1, st)

        for ch in [int(c) for c in args.chunks.split(",")]:
            arena.set_param_groups(pg.index, len(pg), chunk_floats=ch)
            arena.write_group_hyper([lr] * len(pg), [wd] * len(pg), 0.9, 1.0)
            table, n_chunks, n_frags = arena.chunk_table(ranges)
            hp = arena.group_hyper.data_ptr()

            def grouped():
                L.gs_sgd_step_groups(pb, gb, mb, table.data_ptr(), n_chunks, hp, 1, st)

            for fn in (base, grouped):            # warm both
                _timed(fn, 3)
            tb, tg = [], []
            for _ in range(args.rounds):
                tb.append(_timed(base, args.reps))
                tg.append(_timed(grouped, args.reps))
            mb_, mg = statistics.median(tb), statistics.median(tg)
            rows.append((name, len(ranges), n_frags, ch, n_chunks, elems * 4 / 1e6, mb_, min(tb), max(tb),
                         mg, min(tg), max(tg), mg / mb_, 24.0 * elems / (mg * 1e-6) / 1e12,
                         24.0 * elems / (mg * 1e-6) / HBM_PEAK))
            print("%-4s ranges %d fragments %3d CH %6d chunks %5d  %7.1f MB  gs_sgd_step %7.1f us "
                  "(%.1f..%.1f)  gs_sgd_step_groups %7.1f us (%.1f..%.1f)  ratio %.3f  %.2f TB/s = %.2f of peak"
                  % rows[-1], flush=True)
    arena.set_param_groups(pg.index, len(pg))
    runner.refresh_active()
    return rows


def bench_steps(args, cfg, runners):
    g = torch.Generator().manual_seed(0)
    batch = dict(img=torch.randn(N, 3, H, W, generator=g).cuda(),
                 img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3),
                                 flip=False) for _ in range(N)],
                 gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda())
    rows = []
    for name in [a for a in args.anchors.split(",") if a]:
        res = {"plain": [], "paramwise": []}
        for r in runners.values():
            r.set_arch(anchor_meta(cfg, name))
        for p in range(args.passes + 1):          # pass 0: warm-up of both
            for kind in ("plain", "paramwise"):
                r = runners[kind]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    r.train_iter(batch)
                torch.cuda.synchronize()
                if p > 0:
                    res[kind].append(N * args.steps / (time.perf_counter() - t0))
        a, b = statistics.median(res["plain"]), statistics.median(res["paramwise"])
        rows.append((name, a, min(res["plain"]), max(res["plain"]), b, min(res["paramwise"]),
                     max(res["paramwise"]), b / a))
        print("%-4s plain %6.2f img/s (%.2f..%.2f)  paramwise %6.2f img/s (%.2f..%.2f)  x%.3f" % rows[-1],
              flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", default="MAX,R50,MIN")
    ap.add_argument("--chunks", default="4096,16384,65536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paramwise.py measures on the MI355X: no GPU found")
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_paramwise.py"))
    grouped = make_runner(cfg, True)
    krows = [] if args.no_kernel else bench_kernel(args, cfg, grouped)
    srows = [] if args.no_steps else bench_steps(args, cfg, dict(plain=make_runner(cfg, False),
                                                                 paramwise=grouped))
    if args.md:
        with open(args.md, "w") as f:
            if krows:
                f.write("| subnet | merged ranges | fragments | CH floats | chunks | MB per buffer | gs_sgd_step us "
                        "(min..max) | gs_sgd_step_groups us (min..max) | ratio | TB/s | of 8 TB/s |\n"
                        "|---|---|---|---|---|---|---|---|---|---|---|\n")
                for r in krows:
                    f.write("| %s | %d | %d | %d | %d | %.1f | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.3f | "
                            "%.2f | %.2f |\n" % r)
            if srows:
                f.write("\n| subnet | plain img/s (min..max) | paramwise img/s (min..max) | ratio |\n|---|---|---|---|\n")
                for r in srows:
                    f.write("| %s | %.2f (%.2f..%.2f) | %.2f (%.2f..%.2f) | %.3f |\n" % r)


if __name__ == "__main__":
    main()
