#!/usr/bin/env python
"""The fused AdamW (gs_adamw_step_groups) measured against the grouped SGD:

    python tools/bench_adamw.py [--families resnet,convnext,vit] [--anchors MIN,MAX] [--chunks 4096]
                                [--rounds 5] [--reps 20] [--steps 10] [--passes 3] [--no-kernel]
                                [--no-steps] [--md out.md]

(a) kernel alone, device events, warmed: per supernet family and anchor, one gs_adamw_step_groups call
    (the step launch and the counter launch) over the subnet's PER-PARAMETER chunk table against one
    gs_sgd_step_groups launch over the same active ranges with the same parameter groups (fragments merged
    across parameters), alternating in one process, --rounds rounds of --reps repetitions; median and
    min..max of the rounds.  Bytes moved: AdamW 32 B per element (read p, g, m, v; write p, m, v, g), SGD
    24 B, so the time ratio to expect at equal bandwidth is 4/3.  (Per round the buffers stay the same:
    the largest subnets exceed the 256 MiB Infinity Cache several times over; the MIN anchors partly fit,
    for both kernels alike.)
(b) training images/s (512x1024 crops, bs 2) of the two AdamW configs against their SGD twins, every
    measurement in a fresh child process (one model per process), the two configs alternating, median of
    --passes.
bench.py (the training headline) is not involved."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

N, H, W = 2, 512, 1024
NORM_ONLY = dict(norm_decay_mult=0.)
# family -> (config the model and anchors come from, AdamW twin config or None, paramwise_cfg of the tables)
FAMILIES = {
    "resnet": ("fcn_ar50to101v2.py", None, NORM_ONLY),
    "convnext": ("upernet_convnext_t2b.py", "upernet_convnext_t2b_adamw.py", NORM_ONLY),
    "vit": ("upernet_elastic_vit.py", "upernet_elastic_vit_adamw.py",
            dict(custom_keys={"pos_embed": dict(decay_mult=0.), "cls_token": dict(decay_mult=0.)},
                 norm_decay_mult=0.)),
}


def load_cfg(name):
    from gaia_seg_amd.core.config import Config
    return Config.fromfile(os.path.join(ROOT, "configs", "supernet", name))


# the smallest and the largest named subnet of a family (the ConvNeXt space names them after the models)
ALIASES = {"convnext": {"MIN": "ConvNeXt-T", "MAX": "ConvNeXt-B"}}


def anchors_of(cfg, family):
    """{MIN / MAX / ...: meta} from the anchors of the train and val samplers"""
    found = {}
    for s in [cfg.val_sampler] + list(cfg.train_sampler.get("model_samplers", [])):
        for m in s.get("anchors", []):
            found[m["name"]] = dict(m)
    for alias, name in ALIASES.get(family, {}).items():
        found[alias] = found[name]
    return found


def make_runner(cfg, optimizer):
    """a runner on a fresh model of ``cfg`` under ``optimizer`` (cfg.lr_config's schedule)"""
    from gaia_seg_amd.apis.train import check_lr_policy
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner,
                                          PolyLrUpdaterHook)
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    opt = check_optimizer_cfg(optimizer)
    if opt.get("type", "SGD") == "AdamW":
        arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=opt.get("momentum", 0.0), weight_decay=opt.get("weight_decay", 0.0),
                             max_iters=10 ** 6, param_groups=build_param_groups(model, optimizer))
    policy, lrc = check_lr_policy(cfg)
    runner.register_hook(PolyLrUpdaterHook(**lrc) if policy == "poly" else FixedLrUpdaterHook(**lrc))
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


def bench_kernel(args, family):
    """one model, one arena switched between the two optimizer kinds (its tables follow the kind)"""
    from gaia_seg_amd.core.optimizer import build_param_groups
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    base_cfg, _, pw = FAMILIES[family]
    cfg = load_cfg(base_cfg)
    runner = make_runner(cfg, dict(type="SGD", lr=1e-6, momentum=0.9, weight_decay=5e-4, paramwise_cfg=pw))
    arena, model = runner.arena, runner.model
    pg = build_param_groups(model, dict(type="AdamW", lr=1e-6, weight_decay=0.01, paramwise_cfg=pw))
    L, st = lib.load(), current_stream_ptr()
    anchors = anchors_of(cfg, family)
    rows = []
    for name in [a for a in args.anchors.split(",") if a]:
        runner.set_arch(anchors[name])
        ranges = list(runner.active_ranges)
        elems = sum(b - a for a, b in ranges)
        for ch in [int(c) for c in args.chunks.split(",")]:
            arena.set_optimizer("SGD")
            arena.set_param_groups(pg.index, len(pg), chunk_floats=ch)
            arena.write_group_hyper([1e-6] * len(pg), [5e-4] * len(pg), 0.9, 1.0)
            s_table, s_chunks, s_frags = arena.chunk_table(ranges)
            pb, gb, mb = arena.flat_param.data_ptr(), arena.flat_grad.data_ptr(), arena.flat_mom.data_ptr()
            s_hyper = arena.group_hyper

            def sgd():
                L.gs_sgd_step_groups(pb, gb, mb, s_table.data_ptr(), s_chunks, s_hyper.data_ptr(), 1, st)

            arena.set_optimizer("AdamW", (0.9, 0.999), 1e-8)
            arena.write_adamw_hyper([1e-6] * len(pg), [0.01] * len(pg), 1.0)
            a_table, a_chunks, a_frags = arena.chunk_table(ranges)
            vb, sb, a_hyper = arena.flat_var.data_ptr(), arena.steps.data_ptr(), arena.adamw_hyper
            n_slots = arena.steps.numel()
            small = int((a_table[:, 1] < 256).sum())      # chunks of fewer than 256 float4: not one per thread

            def adamw():
                L.gs_adamw_step_groups(pb, gb, mb, vb, sb, n_slots, a_table.data_ptr(), a_chunks,
                                       a_hyper.data_ptr(), 1, st)

            for fn in (sgd, adamw):
                _timed(fn, 3)
            ts, ta = [], []
            for _ in range(args.rounds):
                ts.append(_timed(sgd, args.reps))
                ta.append(_timed(adamw, args.reps))
            ms, ma = statistics.median(ts), statistics.median(ta)
            rows.append((family, name, ch, elems * 4 / 1e6, s_frags, s_chunks, a_frags, a_chunks, small,
                         ms, min(ts), max(ts), 24.0 * elems / (ms * 1e-6) / 1e9,
                         ma, min(ta), max(ta), 32.0 * elems / (ma * 1e-6) / 1e9, ma / ms))
            print("%-8s %-4s CH %6d %7.1f MB/buffer  SGD frags %4d chunks %5d | AdamW params %4d chunks %5d "
                  "(%d short)  sgd %7.1f us (%.1f..%.1f) %6.0f GB/s  adamw %7.1f us (%.1f..%.1f) %6.0f GB/s  "
                  "ratio %.3f" % rows[-1], flush=True)
            arena.reset_optimizer_state()
    arena.set_optimizer("SGD")
    arena.set_param_groups(pg.index, len(pg))
    del runner, arena, model
    torch.cuda.empty_cache()
    return rows


def steps_child(args, family, kind):
    """one process, one model: images/s of config ``kind`` per anchor, one JSON line"""
    base_cfg, adamw_cfg, _ = FAMILIES[family]
    cfg = load_cfg(adamw_cfg if kind == "adamw" else base_cfg)
    runner = make_runner(cfg, cfg.optimizer)
    anchors = anchors_of(cfg, family)
    g = torch.Generator().manual_seed(0)
    batch = dict(img=torch.randn(N, 3, H, W, generator=g).cuda(),
                 img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3),
                                 flip=False) for _ in range(N)],
                 gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda())
    out = {}
    for name in [a for a in args.anchors.split(",") if a]:
        runner.set_arch(anchors[name])
        for _ in range(3):                         # warm-up
            runner.train_iter(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            runner.train_iter(batch)
        torch.cuda.synchronize()
        out[name] = N * args.steps / (time.perf_counter() - t0)
    print("RESULT " + json.dumps(out), flush=True)


def bench_steps(args, family):
    """Every measurement in a process of its own, the two configs alternating: a second model built in one
    process trains at another speed than the first (0.86-1.0 of it on the ViT, whichever optimizer either
    has), which an in-process A/B would book as the optimizer's."""
    if FAMILIES[family][1] is None:
        return []
    res = {}
    for p in range(args.passes):
        for kind in ("sgd", "adamw"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "%s,%s" % (family, kind),
                   "--anchors", args.anchors, "--steps", str(args.steps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                raise SystemExit("child %s failed (exit %d):\n%s" % (cmd[3:], r.returncode, r.stderr[-2000:]))
            for name, v in json.loads(line[-1][7:]).items():
                res.setdefault(name, {"sgd": [], "adamw": []})[kind].append(v)
    rows = []
    for name, r in res.items():
        a, b = statistics.median(r["sgd"]), statistics.median(r["adamw"])
        rows.append((family, name, a, min(r["sgd"]), max(r["sgd"]), b, min(r["adamw"]), max(r["adamw"]), b / a))
        print("%-8s %-4s SGD %6.2f img/s (%.2f..%.2f)  AdamW %6.2f img/s (%.2f..%.2f)  x%.3f" % rows[-1],
              flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="resnet,convnext,vit")
    ap.add_argument("--anchors", default="MIN,MAX")
    ap.add_argument("--chunks", default="4096", help="chunk sizes in floats (the arena's is 4096)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--child", default=None, help="internal: 'family,kind' measured in this process")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw.py measures on the MI355X: no GPU found")
    if args.child:
        return steps_child(args, *args.child.split(","))
    krows, srows = [], []
    for family in [f for f in args.families.split(",") if f]:
        if not args.no_kernel:
            krows += bench_kernel(args, family)
        if not args.no_steps:
            srows += bench_steps(args, family)
    if args.md:
        with open(args.md, "w") as f:
            if krows:
                f.write("| supernet | subnet | CH floats | MB per buffer | SGD fragments | SGD chunks | AdamW parameters | AdamW chunks "
                        "| short chunks | gs_sgd_step_groups us (min..max) | GB/s | gs_adamw_step_groups us "
                        "(min..max) | GB/s | ratio |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
                for r in krows:
                    f.write("| %s | %s | %d | %.1f | %d | %d | %d | %d | %d | %.1f (%.1f..%.1f) | %.0f | "
                            "%.1f (%.1f..%.1f) | %.0f | %.3f |\n" % r)
            if srows:
                f.write("\n| supernet | subnet | SGD img/s (min..max) | AdamW img/s (min..max) | ratio |\n"
                        "|---|---|---|---|---|\n")
                for r in srows:
                    f.write("| %s | %s | %.2f (%.2f..%.2f) | %.2f (%.2f..%.2f) | %.3f |\n" % r)


if __name__ == "__main__":
    main()
