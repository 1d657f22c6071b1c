#!/usr/bin/env python
"""Elastic input resolution (gs_batch_rescale, apply_input_shape) measured on
the FCN supernet at 1024x512, bs 2:

    python tools/bench_input_shape.py [--scales 480,640,800] [--rounds 7] [--reps 50] [--steps 30]
                                      [--passes 5] [--no-kernel] [--no-steps]
                                      [--parent-bench a.json,..] [--this-bench b.json,..] [--md out.md]

(a) kernel alone, device events, warmed: one gs_batch_rescale launch (image and labels) from 512x1024
    to each scale, next to a device-to-device copy of the same OUTPUT bytes (12 B of image + 8 B of
    labels per output pixel), alternating in one process, --rounds rounds of --reps repetitions each;
    median and the min..max spread of the rounds.  The kernel also READS the touched part of the
    source, so bytes moved = output bytes + min(source bytes, 4 taps per output element); the rate
    is given on the output bytes alone (what the copy moves once in each direction).
(b) R50 training images/s with the flag at each scale and on the scale-sampled mix (the reference's
    seven candidates 480..960, in a seeded order), next to the fixed-size run (flag off) of the same
    runner, passes alternating, median of --passes.  A rate at scale S counts images, not pixels:
    (S / 512)^2 times the pixels per image.
(c) the default path: --parent-bench / --this-bench take bench.py result files (one JSON line each) of
    the parent commit and of this one, run alternating on one box, and the table lists them.
bench.py (the training headline) is not involved in (a) and (b)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.core.model_space import resolve_input_shape  # noqa: E402

N, H, W = 2, 512, 1024
MIX = (480, 560, 640, 720, 800, 880, 960)


def _batch():
    g = torch.Generator().manual_seed(0)
    return dict(img=torch.randn(N, 3, H, W, generator=g).cuda(),
                img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3),
                                flip=False, scale_factor=1.0) for _ in range(N)],
                gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda())


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per call


def bench_kernel(args, batch):
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    L = lib.load()
    img, gt = batch["img"], batch["gt_semantic_seg"]
    rows = []
    for s in args.scales:
        h2, w2 = resolve_input_shape(s, H, W)
        out = torch.empty((N, 3, h2, w2), dtype=torch.float32, device="cuda")
        out_gt = torch.empty((N, 1, h2, w2), dtype=torch.int64, device="cuda")
        nbytes = out.numel() * 4 + out_gt.numel() * 8
        src, dst = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))
        st = current_stream_ptr()

        def rescale():
            lib.check(L.gs_batch_rescale(img.data_ptr(), gt.data_ptr(), N, H, W, out.data_ptr(),
                                         out_gt.data_ptr(), h2, w2, st), "gs_batch_rescale")

        def copy():
            dst.copy_(src)

        for fn in (rescale, copy):                # warm both
            _timed(fn, 5)
        tr, tc = [], []
        for _ in range(args.rounds):
            tr.append(_timed(rescale, args.reps))
            tc.append(_timed(copy, args.reps))
        mr, mc = statistics.median(tr), statistics.median(tc)
        rows.append((s, h2, w2, nbytes / 1e6, mr, min(tr), max(tr), mc, min(tc), max(tc), mr / mc,
                     nbytes / (mr * 1e-6) / 1e12))
        print("scale %4d -> %4dx%-4d  %6.1f MB out  gs_batch_rescale %6.1f us (%.1f..%.1f)  copy %6.1f us "
              "(%.1f..%.1f)  ratio %.2f  %.2f TB/s of output" % rows[-1], flush=True)
    return rows


def make_runner(cfg):
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, PolyLrUpdaterHook
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    opt = dict(cfg.optimizer)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=opt["momentum"], weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             apply_input_shape=True)
    lrc = dict(cfg.lr_config)
    lrc.pop("policy")
    runner.register_hook(PolyLrUpdaterHook(**lrc))
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner


def bench_steps(args, cfg, batch):
    runner = make_runner(cfg)
    r50 = next(dict(m) for m in cfg.train_sampler["model_samplers"][0]["anchors"] if m.get("name") == "R50")
    mix = list(MIX) * max(1, args.steps // len(MIX))
    random.Random(0).shuffle(mix)
    # kind -> the data.input_shape of each of its steps (None: no key, flag off)
    kinds = [("fixed 512 (flag off)", [None] * args.steps)] + \
            [("scale %d" % s, [s] * args.steps) for s in args.scales] + \
            [("mix %d..%d" % (MIX[0], MIX[-1]), mix)]
    res = {k: [] for k, _ in kinds}
    for p in range(args.passes + 1):              # pass 0: one step per shape warms it
        for kind, seq in kinds:
            if p == 0:
                seq = sorted(set(seq), key=lambda v: v or 0)
            runner.apply_input_shape = seq[0] is not None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v in seq:
                runner.set_arch(r50 if v is None else dict(r50, **{"data.input_shape": v}))
                runner.train_iter(batch)
            torch.cuda.synchronize()
            if p > 0:
                res[kind].append(N * len(seq) / (time.perf_counter() - t0))
    base = statistics.median(res[kinds[0][0]])
    rows = []
    for kind, seq in kinds:
        v = res[kind]
        sizes = [(H, W) if s is None else resolve_input_shape(s, H, W) for s in seq]
        px = statistics.mean(h2 * w2 / (H * W) for h2, w2 in sizes)
        rows.append((kind, statistics.median(v), min(v), max(v), statistics.median(v) / base, px))
        print("%-22s %7.2f img/s (%.2f..%.2f)  x%.3f of fixed, %.2fx the pixels per image" % rows[-1],
              flush=True)
    return rows


def bench_files(paths):
    vals = []
    for p in [q for q in (paths or "").split(",") if q]:
        with open(p) as fh:
            lines = [ln for ln in fh.read().splitlines() if ln.strip().startswith("{")]
        vals.append(json.loads(lines[-1])["value"])
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="480,640,800")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--parent-bench", default=None)
    ap.add_argument("--this-bench", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    args.scales = [int(s) for s in args.scales.split(",") if s]
    parent, this = bench_files(args.parent_bench), bench_files(args.this_bench)
    krows = srows = []
    if not (args.no_kernel and args.no_steps):
        if not torch.cuda.is_available():
            raise SystemExit("bench_input_shape.py measures on the MI355X: no GPU found")
        from gaia_seg_amd.core.config import Config
        cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
        batch = _batch()
        krows = [] if args.no_kernel else bench_kernel(args, batch)
        srows = [] if args.no_steps else bench_steps(args, cfg, batch)
    if parent or this:
        print("bench.py images/s  parent: %s  this: %s" % (parent, this))
    if args.md:
        with open(args.md, "w") as f:
            if krows:
                f.write("| scale | output | MB written | gs_batch_rescale us (min..max) | copy us (min..max) | "
                        "ratio | TB/s of output |\n|---|---|---|---|---|---|---|\n")
                for r in krows:
                    f.write("| %d | %dx%d | %.1f | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.2f | %.2f |\n" % r)
            if srows:
                f.write("\n| R50, bs 2 | img/s (min..max) | of the fixed-size run | pixels per image |\n"
                        "|---|---|---|---|\n")
                for r in srows:
                    f.write("| %s | %.2f (%.2f..%.2f) | %.3f | %.2fx |\n" % r)
            if parent or this:
                f.write("\n| bench.py run | parent images/s | this commit images/s |\n|---|---|---|\n")
                for i in range(max(len(parent), len(this))):
                    f.write("| %d | %s | %s |\n" % (i + 1, parent[i] if i < len(parent) else "-",
                                                   this[i] if i < len(this) else "-"))
                if parent and this:
                    f.write("| median | %.3f | %.3f |\n" % (statistics.median(parent), statistics.median(this)))


if __name__ == "__main__":
    main()
