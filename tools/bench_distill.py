#!/usr/bin/env python
"""In-place distillation on the GPU (HIP events):
  * ms per sandwich iteration (MAX + MIN + 3 random members, one SGD step) and per member at BASELINE
    config 3 (configs/supernet/pspnet_ar50to101v2_inplace_distill.py: 1024x512 crops, bs 2), next to
    the ordinary one-subnet step of the same config;
  * us per fused KD forward / backward call at the config-3 head shapes (16x32 and 32x64 logits) and
    the OS8 shape (64x128), 19 classes, N = 2, with interpolation to 512x1024 and without;
  * the gradient-accumulation kernel over the config-3 arena: us and GB/s for 16 bytes per element
    (two reads, two writes).

    python tools/bench_distill.py [--iters 5] [--warmup 2] [--md out.md]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402
from gaia_seg_amd.models.losses.distill_loss import kd_desc  # noqa: E402


def _time(fn, iters):
    fn()
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return b.elapsed_time(e) / iters


def bench_kd(iters):
    L = lib.load()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, n, h, w, H, W in [("config 3 decode (x32)", 2, 16, 32, 512, 1024),
                                ("config 3 aux (x16)", 2, 32, 64, 512, 1024),
                                ("OS8 decode / aux (x8)", 2, 64, 128, 512, 1024)]:
        for interp in (True, False):
            torch.manual_seed(0)
            ld = 20
            s = torch.randn(n, h, w, ld, device=dev).permute(0, 3, 1, 2)[:, :19]
            t = torch.randn(n, h, w, ld, device=dev).permute(0, 3, 1, 2)[:, :19]
            d = kd_desc(s, t, (H, W), 2.0, False, interp)
            lse_s = torch.empty(n, d.H, d.W, device=dev)
            lse_t = torch.empty_like(lse_s)
            out = torch.empty(1, device=dev)
            nb = max(L.gs_kd_workspace_bytes(ctypes.byref(d)), L.gs_kd_backward_workspace_bytes(ctypes.byref(d), ld))
            ws = torch.empty(nb // 4 + 64, device=dev)
            buf = torch.empty(n, h, w, ld, device=dev)

            def fwd():
                lib.check(L.gs_kd_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                          lse_t.data_ptr(), 1e-4, out.data_ptr(), ws.data_ptr(),
                                          ws.numel() * 4, st), "gs_kd_forward")

            def bwd():
                lib.check(L.gs_kd_backward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                           lse_t.data_ptr(), 1e-4, buf.data_ptr(), ld, ws.data_ptr(),
                                           ws.numel() * 4, st), "gs_kd_backward")
            rows.append((name, "%dx%d -> %dx%d" % (h, w, d.H, d.W), 1000 * _time(fwd, iters),
                         1000 * _time(bwd, iters)))
    return rows


def _runner(cfg, sandwich):
    from gaia_seg_amd.apis import sandwich_train_sampler
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner,
                                          ManipulateArchHook, SandwichHook)
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.01,
                             momentum=0.9, weight_decay=5e-4, max_iters=10 ** 6)
    runner.register_hook(FixedLrUpdaterHook())
    if sandwich:
        sampler = build_model_sampler(sandwich_train_sampler(cfg))
        sampler.seed(0)
        runner.register_hook(SandwichHook(sampler, cfg.get("distill_cfg")))
    else:
        sampler = build_model_sampler(cfg.train_sampler)
        sampler.seed(0)
        runner.register_hook(ManipulateArchHook(sampler))
        runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner, arena


def bench_iterations(iters, warmup):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.synthetic import make_batch
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_inplace_distill.py"))
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    out = {}
    # the ordinary step of config 3 (one sampled subnet per iteration)
    runner, _ = _runner(cfg, sandwich=False)
    for _ in range(warmup):
        runner.train_iter(batch)
    out["mixed_step_ms"] = _time(lambda: runner.train_iter(batch), iters)
    del runner
    torch.cuda.empty_cache()
    # sandwich iterations, with an event after every member's gradient move
    runner, arena = _runner(cfg, sandwich=True)
    marks = []
    orig = arena.accumulate

    def accumulate(ranges, into="buffer"):
        orig(ranges, into)
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((into, e))
    arena.accumulate = accumulate
    for _ in range(warmup):
        runner.train_iter(batch)
    per_member, names, total = None, None, 0.0
    for _ in range(iters):
        marks.clear()
        b = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        b.record()
        res = runner.train_iter(batch)
        e.record()
        torch.cuda.synchronize()
        total += b.elapsed_time(e)
        ev = [b] + [m for k, m in marks if k == "buffer"]
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(ev) - 1)]
        per_member = ms if per_member is None else [a + c for a, c in zip(per_member, ms)]
        names = res["members"]
    out["sandwich_ms"] = total / iters
    out["members"] = list(zip(names, [v / iters for v in per_member]))
    # the accumulation kernel over the whole arena
    rng = [(0, arena.numel)]
    arena.accumulate = orig
    us = 1000 * _time(lambda: arena.accumulate(rng, "buffer"), 20)
    out["accumulate"] = (arena.numel, us, 16.0 * arena.numel / (us * 1e-6) / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kd-iters", type=int, default=30)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    lib.load()
    lines = ["# In-place distillation on the MI355X (tools/bench_distill.py)", ""]
    it = bench_iterations(args.iters, args.warmup)
    lines += ["## Sandwich iteration, config 3 (1024x512, bs 2, %d iterations after %d warm-up)"
              % (args.iters, args.warmup), "",
              "| | ms |", "|---|---|",
              "| ordinary step (one sampled subnet) | %.1f |" % it["mixed_step_ms"],
              "| sandwich iteration (all members + one SGD step) | %.1f |" % it["sandwich_ms"]]
    lines += ["| member %s (forward + backward + gradient move) | %.1f |" % (n, v) for n, v in it["members"]]
    lines += ["", "sandwich / ordinary step: %.2fx" % (it["sandwich_ms"] / it["mixed_step_ms"]), ""]
    n, us, gbs = it["accumulate"]
    lines += ["## Gradient accumulation kernel", "",
              "%d elements (16 B each: 2 reads + 2 writes): %.1f us, %.0f GB/s" % (n, us, gbs), ""]
    lines += ["## Fused KD kernels (19 classes, N = 2, T = 2)", "",
              "| shape | evaluation grid | forward us | backward us |", "|---|---|---|---|"]
    lines += ["| %s | %s | %.1f | %.1f |" % r for r in bench_kd(args.kd_iters)]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
