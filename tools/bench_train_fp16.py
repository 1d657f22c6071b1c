#!/usr/bin/env python
"""Training throughput of the FCN supernet (configs/supernet/fcn_ar50to101v2.py, 1024x512 crops, bs 2)
in fp32 and in fp16 (conv operands, static loss scale 512: core/runner.py Fp16ArenaOptimizerHook):

    python tools/bench_train_fp16.py [--anchors MIN,R50,MAX] [--mix] [--steps 10] [--passes 5]
                                     [--shapes] [--md out.md]

Per anchor (and the train sampler's mix with --mix): images/s, fp32 and fp16 passes alternating in
one process, median of --passes; and the share of the conv FLOPs (2*M*N*K) per step that ran on the
f16 loop, forward and data gradient apart (of all conv FLOPs of the step, weight gradients included).
--shapes adds the data gradient of every R50 / MAX / MIN bottleneck conv shape at the bench workload,
kernel alone (HIP events, 30 launches), fp32 loop against f16, with the K loop taken.
bench.py (the training headline) is not involved."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

KLOOP = {0: "generic", 1: "fp32", 2: "fp32x2", 3: "bf16x3", 4: "stream", 5: "f16"}
RES = [(128, 256), (64, 128), (32, 64), (16, 32)]     # stage resolutions of a 512x1024 crop
WIDTHS = {"R50": [64, 128, 256, 512], "MAX": [80, 160, 320, 640], "MIN": [48, 96, 192, 384]}
N, H, W = 2, 512, 1024


def anchor_meta(cfg, name):
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:
        if m.get("name") == name:
            return dict(m)
    raise KeyError(name)


def flops(L):
    buf = (ctypes.c_double * (3 * lib.KLOOP_COUNT))()
    L.gs_debug_conv_launch_flops(buf, 1)
    f16 = (ctypes.c_double * 2)()
    L.gs_debug_f16_launches_by_op(None, f16, 1)
    L.gs_debug_f16_launches(None, None, 1)
    # (f16 launches are not in the per-K-loop tables: the step's conv FLOPs are both together)
    return sum(buf) + f16[0] + f16[1], f16[0], f16[1]


def make_runner(cfg):
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, ManipulateArchHook
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.01,
                             momentum=0.9, weight_decay=5e-4, max_iters=10 ** 6)
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    hook = ManipulateArchHook(build_model_sampler(cfg.train_sampler))
    return runner, hook


def bench_steps(args, L, cfg):
    runner, mix_hook = make_runner(cfg)
    g = torch.Generator().manual_seed(0)
    batch = dict(img=torch.randn(N, 3, H, W, generator=g).cuda(),
                 img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3),
                                 flip=False) for _ in range(N)],
                 gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda())
    names = [a for a in args.anchors.split(",") if a] + (["mix"] if args.mix else [])
    rows = []
    for name in names:
        if name == "mix":
            runner.hooks.append(mix_hook)
        else:
            runner.set_arch(anchor_meta(cfg, name))
        res = {"fp32": [], "fp16": []}
        share = {}
        for p in range(args.passes + 1):          # pass 0: warm-up of both precisions
            for prec in ("fp32", "fp16"):
                runner.train_precision = prec
                runner.loss_scale = 512.0 if prec == "fp16" else 1.0
                random.seed(p)
                np.random.seed(p)
                torch.cuda.synchronize()
                flops(L)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    runner.train_iter(batch)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                tot, f_fwd, f_dg = flops(L)
                if p > 0:
                    res[prec].append(N * args.steps / dt)
                    share[prec] = (f_fwd / tot, f_dg / tot)
        if name == "mix":
            runner.hooks.remove(mix_hook)
        runner.train_precision, runner.loss_scale = "fp32", 1.0
        a, b = statistics.median(res["fp32"]), statistics.median(res["fp16"])
        rows.append((name, a, b, b / a, share["fp16"][0], share["fp16"][1]))
        print("%-4s fp32 %6.2f img/s  fp16 %6.2f img/s  x%.3f  f16 share of conv FLOPs: fwd %.3f dgrad "
              "%.3f   (fp32 passes %s, fp16 passes %s)" % (rows[-1] + (
                  " ".join("%.1f" % v for v in res["fp32"]), " ".join("%.1f" % v for v in res["fp16"]))),
              flush=True)
    return rows


def bench_shapes(args, L):
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    dev = torch.device("cuda")
    st = current_stream_ptr()
    rows = []
    for wname in [a for a in args.anchors.split(",") if a in WIDTHS]:
        ws = WIDTHS[wname]
        for s, (h, w) in enumerate(RES):
            wd = ws[s]
            cases = [("%s s%d conv2 3x3 %d" % (wname, s + 1, wd), h, w, wd, wd, 3, 1),
                     ("%s s%d conv3 1x1 %d->%d" % (wname, s + 1, wd, 4 * wd), h, w, wd, 4 * wd, 1, 1),
                     ("%s s%d conv1 1x1 %d->%d" % (wname, s + 1, 4 * wd, wd), h, w, 4 * wd, wd, 1, 1)]
            if s > 0:
                ph, pw = RES[s - 1]
                cases.append(("%s s%d.0 conv2 3x3/2 %d" % (wname, s + 1, wd), ph, pw, wd, wd, 3, 2))
            for name, hh, ww, ci, co, k, stride in cases:
                d = lib.conv_desc(N, hh, ww, ci, co, k, stride)
                dy = torch.randn(N, d.Ho, d.Wo, co, device=dev)
                dx = torch.empty(N, hh, ww, ci, device=dev)
                wt = torch.randn(k, k, ci, co, device=dev) * 0.05
                need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
                wsb = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
                fl = 2.0 * N * hh * ww * ci * co * k * k / (stride * stride)
                out = [name]
                for mode in (0, 1):
                    L.gs_set_train_precision(mode)
                    try:
                        def run():
                            return L.gs_conv2d_dgrad(ctypes.byref(d), dy.data_ptr(), wt.data_ptr(),
                                                     dx.data_ptr(), 0, wsb.data_ptr(), wsb.numel(), st)
                        for _ in range(5):
                            lib.check(run(), "dgrad")
                        rec = lib.DebugLaunch()
                        L.gs_debug_last_conv_launch(ctypes.byref(rec))
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(30):
                            run()
                        e1.record()
                        torch.cuda.synchronize()
                    finally:
                        L.gs_set_train_precision(0)
                    us = e0.elapsed_time(e1) * 1e3 / 30
                    out += [us, fl / us / 1e6, "%s %dx%d s%d" % (KLOOP.get(rec.kloop, "?"), rec.bm, rec.bn,
                                                               rec.splits)]
                out.append(out[1] / out[4])
                rows.append(tuple(out))
                print("%-28s fp32 %7.1f us %6.1f TF %-18s f16 %7.1f us %6.1f TF %-18s x%.2f" % rows[-1],
                      flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", default="MIN,R50,MAX")
    ap.add_argument("--mix", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    from gaia_seg_amd.core.config import Config
    L = lib.load()
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
    srows = bench_shapes(args, L) if args.shapes else []
    arows = [] if args.no_steps else bench_steps(args, L, cfg)
    if args.md:
        with open(args.md, "w") as f:
            if arows:
                f.write("| subnet | fp32 img/s | fp16 img/s | speed-up | f16 share of conv FLOPs: fwd | dgrad |\n"
                        "|---|---|---|---|---|---|\n")
                for r in arows:
                    f.write("| %s | %.2f | %.2f | %.3f | %.3f | %.3f |\n" % r)
            if srows:
                f.write("\n| dgrad shape (%dx%d, bs %d) | fp32 us | fp32 TF | fp32 kernel | f16 us | f16 TF | "
                        "f16 kernel | speed-up |\n|---|---|---|---|---|---|---|---|\n" % (H, W, N))
                for r in srows:
                    f.write("| %s | %.1f | %.1f | %s | %.1f | %.1f | %s | %.2f |\n" % r)


if __name__ == "__main__":
    main()
