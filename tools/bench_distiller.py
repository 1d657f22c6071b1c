#!/usr/bin/env python
"""Fixed-teacher distillation (DynamicDistiller) on the GPU, HIP events throughout:
  * the two loss operators alone (gs_distill_*, gs_pairwise_*): us per forward / backward call and
    the launches each makes, at the shapes of the PSP supernet at 1024x512, bs 2;
  * images/s of the distilled training step (R50 and MIN students under the MAX teacher,
    configs/supernet/pspnet_ar50to101v2_distiller.py) next to two yardsticks that run the code paths a
    plain model has always taken: the DynamicEncoderDecoder step of the same student, and the
    teacher's eval forward on the same batch;
  * with both losses switched off, an interleaved A/B of the distiller's step against the plain step.

    python tools/bench_distiller.py [--iters 8] [--warmup 3] [--ab-runs 5] [--md out.md]"""
import argparse
import ctypes
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402
from gaia_seg_amd.models.losses.distill_loss import distill_desc, pairwise_desc  # noqa: E402

# launches per C-ABI call (csrc/distill.hip): they do not depend on N, P, C or the resolution
LAUNCHES = {"gs_distill_forward": 2, "gs_distill_backward": 2, "gs_pairwise_forward": 3,
            "gs_pairwise_backward": 3}


def _time(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return b.elapsed_time(e) / iters


def bench_ops(iters):
    L = lib.load()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    torch.manual_seed(0)
    for name, hs, ht in [("OS32 student, OS32 teacher", (16, 32), (16, 32)),
                         ("OS32 student, OS8 teacher", (16, 32), (64, 128)),
                         ("OS8 student, OS32 teacher", (64, 128), (16, 32))]:
        n, ld, hw = 2, 20, (512, 1024)
        s = torch.randn(n, hs[0], hs[1], ld, device=dev).permute(0, 3, 1, 2)[:, :19]
        t = torch.randn(n, ht[0], ht[1], ld, device=dev).permute(0, 3, 1, 2)[:, :19]
        d = distill_desc(s, t, hw, 1.0, False)
        lse_s = torch.empty(n, hw[0], hw[1], device=dev)
        lse_t = torch.empty_like(lse_s)
        out = torch.empty(1, device=dev)
        nb = max(L.gs_distill_workspace_bytes(ctypes.byref(d)),
                 L.gs_distill_backward_workspace_bytes(ctypes.byref(d), ld))
        ws = torch.empty(nb // 4 + 64, device=dev)
        buf = torch.empty(n, hs[0], hs[1], ld, device=dev)

        def fwd():
            lib.check(L.gs_distill_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                           lse_t.data_ptr(), 1e-6, out.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 4, st), "gs_distill_forward")

        def bwd():
            lib.check(L.gs_distill_backward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                            lse_t.data_ptr(), 1e-6, buf.data_ptr(), ld, ws.data_ptr(),
                                            ws.numel() * 4, st), "gs_distill_backward")
        rows.append(("distill: " + name, "%dx%d, %dx%d -> %dx%d" % (hs + ht + hw), 1000 * _time(fwd, iters),
                     LAUNCHES["gs_distill_forward"], 1000 * _time(bwd, iters), LAUNCHES["gs_distill_backward"]))
    for name, cs, ct, h, w in [("R50 student under MAX", 2048, 2560, 16, 32),
                               ("MIN student under MAX", 1536, 2560, 16, 32),
                               ("the cap: P = 128", 2048, 2560, 256, 4)]:
        n = 2
        s = torch.relu(torch.randn(n, h, w, cs, device=dev)).permute(0, 3, 1, 2)
        t = torch.relu(torch.randn(n, h, w, ct, device=dev)).permute(0, 3, 1, 2)
        win = (h // 4, h // 4 + h // 2, w // 2, w // 2 + 1)
        d = pairwise_desc(s, t, win, 1.0)
        save = torch.empty(L.gs_pairwise_save_bytes(ctypes.byref(d)) // 8 + 1, dtype=torch.float64, device=dev)
        out = torch.empty(1, device=dev)
        buf = torch.empty(n, h, w, cs, device=dev)

        def fwd():
            lib.check(L.gs_pairwise_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), 1e-2, out.data_ptr(),
                                            save.data_ptr(), save.numel() * 8, st), "gs_pairwise_forward")

        def bwd():
            lib.check(L.gs_pairwise_backward(ctypes.byref(d), s.data_ptr(), save.data_ptr(), save.numel() * 8,
                                             1e-2, buf.data_ptr(), cs, st), "gs_pairwise_backward")
        rows.append(("pairwise: " + name, "Cs %d, Ct %d, %dx%d, P %d" % (cs, ct, h, w, win[1] - win[0]),
                     1000 * _time(fwd, iters), LAUNCHES["gs_pairwise_forward"], 1000 * _time(bwd, iters),
                     LAUNCHES["gs_pairwise_backward"]))
    return rows


def anchor(cfg, name):
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:
        if m.get("name") == name:
            return dict(m)
    raise KeyError(name)


def _runner(model, meta):
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner,
                                          ManipulateArchHook)
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.01,
                             momentum=0.9, weight_decay=5e-4, max_iters=10 ** 6)
    runner.register_hook(ManipulateArchHook(build_model_sampler(dict(type="anchor", anchors=[meta]))))
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner


def bench_steps(args):
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller.py"))
    plain_cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2.py"))
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    tmp = tempfile.mkdtemp()
    ck = os.path.join(tmp, "teacher.pth")
    tcfg = dict(cfg.model["teacher_segmentor"], test_cfg=dict(mode="whole"))
    save_checkpoint(build_segmentor(tcfg), ck)       # random weights: the timing does not depend on them

    def build(c, **over):
        m = dict(c.model)
        m.update(over)
        torch.manual_seed(0)
        return build_segmentor(m, train_cfg=c.get("train_cfg"), test_cfg=c.get("test_cfg")).cuda().train()
    plain = build(plain_cfg)
    dist_ = build(cfg, teacher_ckpt=ck)
    off = build(cfg, teacher_ckpt=None, has_distill_loss=False, has_pairwise_loss=False)
    teacher = dist_.teacher_segmentor
    out = {"students": []}

    def teacher_fwd():
        with torch.no_grad():
            x = teacher.extract_feat(batch["img"])
            teacher._decode_head_forward_test(x, batch["img_metas"])
    out["teacher_ms"] = _time(teacher_fwd, args.iters, args.warmup)
    np.random.seed(0)
    from gaia_seg_amd.core.model_space import build_model_sampler
    first = anchor(cfg, "R50")
    rp, rd, ro = _runner(plain, first), _runner(dist_, first), _runner(off, first)
    for name in ("R50", "MIN"):
        for r in (rp, rd, ro):     # (hooks[0] is the ManipulateArchHook: one anchor per student)
            r.hooks[0].sampler = build_model_sampler(dict(type="anchor", anchors=[anchor(cfg, name)]))
        plain_ms = _time(lambda: rp.train_iter(batch), args.iters, args.warmup)
        dist_ms = _time(lambda: rd.train_iter(batch), args.iters, args.warmup)
        ab = {"plain": [], "off": []}
        for _ in range(args.ab_runs):      # interleaved: plain, flags-off, plain, ...
            ab["plain"].append(_time(lambda: rp.train_iter(batch), args.iters, 1))
            ab["off"].append(_time(lambda: ro.train_iter(batch), args.iters, 1))
        out["students"].append(dict(name=name, plain_ms=plain_ms, dist_ms=dist_ms, ab=ab))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=30)
    ap.add_argument("--ab-runs", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    lib.load()
    lines = ["# Fixed-teacher distillation on the MI355X (tools/bench_distiller.py)", "",
             "## The loss operators alone (N = 2, 19 classes; %d calls each)" % args.op_iters, "",
             "| operator | shape | forward us | launches | backward us | launches |", "|---|---|---|---|---|---|"]
    ops_rows = bench_ops(args.op_iters)
    lines += ["| %s | %s | %.1f | %d | %.1f | %d |" % r for r in ops_rows]
    lines += ["", "The autograd wrappers add one elementwise launch per backward (the upstream scalar, applied "
              "on the device).", ""]
    if not args.skip_steps:
        st = bench_steps(args)
        n = 2.0
        lines += ["## Training step, PSP supernet, 1024x512, bs 2 (%d iterations after %d warm-up)"
                  % (args.iters, args.warmup), "",
                  "Teacher (MAX) eval forward on the batch: %.1f ms (%.1f images/s)."
                  % (st["teacher_ms"], 1000 * n / st["teacher_ms"]), "",
                  "| student | plain step ms (img/s) | distilled step ms (img/s) | plain + teacher forward ms | "
                  "excess ms |", "|---|---|---|---|---|"]
        for s in st["students"]:
            both = s["plain_ms"] + st["teacher_ms"]
            lines.append("| %s | %.1f (%.1f) | %.1f (%.1f) | %.1f | %+.1f |"
                         % (s["name"], s["plain_ms"], 1000 * n / s["plain_ms"], s["dist_ms"],
                            1000 * n / s["dist_ms"], both, s["dist_ms"] - both))
        lines += ["", "## Both losses off against the plain step (interleaved A/B, %d runs each, ms per step)"
                  % args.ab_runs, "", "| student | plain | distiller, flags off | sets overlap |", "|---|---|---|---|"]
        for s in st["students"]:
            p, o = s["ab"]["plain"], s["ab"]["off"]
            overlap = not (max(p) < min(o) or max(o) < min(p))
            lines.append("| %s | %s (mean %.2f, spread %.2f) | %s (mean %.2f, spread %.2f) | %s |"
                         % (s["name"], " ".join("%.2f" % v for v in p), sum(p) / len(p), max(p) - min(p),
                            " ".join("%.2f" % v for v in o), sum(o) / len(o), max(o) - min(o),
                            "yes" if overlap else "no"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
