#!/usr/bin/env python
"""The two-length attention operator and the SegFormer supernet on the GPU, HIP events
throughout, at the recipe's 1024x512 crops, bs 2:
  * gs_attention_kv_forward / gs_attention_kv_backward at the four stage shapes of
    configs/supernet/segformer_mit_b1to3_adamw.py's MAX anchor (Nq 32768 / 8192 / 2048 / 512 queries against 512
    keys, 1 / 2 / 5 / 8 heads; K and V as two column slices of one buffer, as the backbone lays them out), with
    the microseconds and the fraction of the fp32 MFMA peak (157.3 TFLOP/s) of the 4 * Nq * Nk * 64 * heads
    forward count and 2.5x that for the backward; beside them, for orientation only, fp32
    torch.nn.functional.scaled_dot_product_attention on the same shapes;
  * the backward with the query split of the dK / dV kernel forced to S = 1 against the planned S, the two
    alternating over --reps repetitions (the delta pre-pass and the dQ kernel are the same launches in both,
    so the difference is the dK / dV kernel's and the combine's), and the workspace bytes of each;
  * the training step (images/s) on the MIN, MID and MAX anchors and on the sampled mix of the train sampler.
Writes its tables to --md (default work_dirs/bench_segformer.md); profiles/r23_segformer.md says which of
them have been measured.

    python tools/bench_segformer.py [--op-iters 20] [--reps 5] [--iters 4] [--warmup 2] [--mix 12]
                                    [--splits 16,32,128] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "segformer_mit_b1to3_adamw.py")
PEAK_TFLOPS = 157.3   # fp32 MFMA (v_mfma_f32_32x32x2_f32) = the fp32 vector rate of the MI355X


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


def _spread(v, fmt="%.1f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(v), min(v), max(v))


def stage_shapes(cfg):
    """[(B, Nq, Nk, heads)] of the MAX arch's four stages at the recipe's crop"""
    bb = cfg.model["backbone"]
    h, w = cfg.crop_size
    out, stride = [], 1
    for s, sr, heads in zip(bb["strides"], bb["sr_ratios"], bb["num_heads"]):
        stride *= s
        hq, wq = h // stride, w // stride
        out.append((cfg.data["samples_per_gpu"], hq * wq, (hq // sr) * (wq // sr), heads))
    return out


def bench_ops(shapes, iters, reps, sweep=()):
    """[(shape, {'fwd' | 'bwd1' | 'bwdS' | 'sdpa_fwd' | 'sdpa_bwd': [us per repetition]}, workspace bytes at
    S = 1, at the plan, planned S)]"""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for b, nq, nk, heads in shapes:
        c = 64 * heads
        q, dq = torch.randn(b, nq, c, device="cuda"), torch.empty(b, nq, c, device="cuda")
        kv, dkv = torch.randn(b, nk, 2 * c, device="cuda"), torch.empty(b, nk, 2 * c, device="cuda")
        o, do = torch.empty(b, nq, c, device="cuda"), torch.randn(b, nq, c, device="cuda")
        lse = torch.empty(b * heads * nq, device="cuda")
        d = lib.attention_kv_desc(b, nq, nk, heads, ldq=c, ldk=2 * c, ldv=2 * c, ldo=c)
        db = ctypes.byref(d)
        need = {}
        try:
            for s in (1, -1):
                lib.check(L.gs_debug_set_attention_kv_split(s), "split")
                need[s] = L.gs_attention_kv_workspace_bytes(db)
            delta = need[1]
            planned = 1 if need[-1] == delta else (need[-1] - delta) // (2 * b * nk * c * 4)
            kp, gp = kv.data_ptr(), dkv.data_ptr()

            def fwd():
                lib.check(L.gs_attention_kv_forward(db, q.data_ptr(), kp, kp + 4 * c, o.data_ptr(), lse.data_ptr(),
                                                    st), "fwd")

            def bwd(s):
                lib.check(L.gs_debug_set_attention_kv_split(s), "split")
                lib.check(L.gs_attention_kv_backward(db, q.data_ptr(), kp, kp + 4 * c, o.data_ptr(), lse.data_ptr(),
                                                     do.data_ptr(), dq.data_ptr(), gp, gp + 4 * c, 0, ws.data_ptr(),
                                                     need[s], st), "bwd")

            # torch's fp32 attention on [B, heads, N, 64] views of the same data (orientation only)
            tq, tk, tv = (t.view(b, -1, heads, 64).transpose(1, 2).contiguous().requires_grad_(True)
                          for t in (q, kv[..., :c], kv[..., c:]))
            tdo = do.view(b, nq, heads, 64).transpose(1, 2).contiguous()
            sdpa = torch.nn.functional.scaled_dot_product_attention

            def sdpa_fwd_bwd():
                sdpa(tq, tk, tv).backward(tdo)

            for s in sweep:   # forced splits beside S = 1 and the plan (--splits)
                lib.check(L.gs_debug_set_attention_kv_split(s), "split")
                need[s] = L.gs_attention_kv_workspace_bytes(db)
            ws = torch.empty(max(need.values()), dtype=torch.uint8, device="cuda")
            us = {k: [] for k in ("fwd", "bwd1", "bwdS", "sdpa_fwd", "sdpa_fwd_bwd") + tuple(sweep)}
            fwd()
            for _ in range(reps):
                us["fwd"].append(1e3 * _time(fwd, iters))
                us["bwd1"].append(1e3 * _time(lambda: bwd(1), iters))
                us["bwdS"].append(1e3 * _time(lambda: bwd(-1), iters))
                for s in sweep:
                    us[s].append(1e3 * _time(lambda: bwd(s), iters))
                with torch.no_grad():
                    us["sdpa_fwd"].append(1e3 * _time(lambda: sdpa(tq, tk, tv), iters))
                us["sdpa_fwd_bwd"].append(1e3 * _time(sdpa_fwd_bwd, iters))
        finally:
            L.gs_debug_set_attention_kv_split(-1)
        rows.append(((b, nq, nk, heads), us, need[1], need[-1], planned))
    return rows


def bench_steps(cfg, args):
    """{anchor or 'mix': images/s} of the recipe's model and optimizer (fixed lr)"""
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    opt = check_optimizer_cfg(cfg.optimizer)
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             param_groups=build_param_groups(model, cfg.optimizer))
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    h, w = cfg.crop_size
    bs = cfg.data["samples_per_gpu"]
    batch = make_batch(bs, h, w, seed=0, device="cuda")
    out = {}
    for meta in cfg.val_sampler["anchors"]:
        runner.set_arch(meta)
        out[meta["name"]] = 1000.0 * bs / _time(lambda: runner.train_iter(batch), args.iters, args.warmup)
    if args.mix > 0:
        import numpy as np
        np.random.seed(0)
        sampler = build_model_sampler(cfg.train_sampler)
        metas = [sampler.sample() for _ in range(args.mix)]

        def mix():
            for meta in metas:
                runner.set_arch(meta)
                runner.train_iter(batch)
        out["mix of %d samples" % args.mix] = 1000.0 * bs * len(metas) / _time(mix, 1, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mix", type=int, default=12)
    ap.add_argument("--splits", default="", help="comma-separated forced splits to time beside S = 1 and the plan")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_segformer.md"))
    args = ap.parse_args()
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_segformer.py measures on the GPU: no device found")
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(CONFIG)
    sweep = tuple(int(v) for v in args.splits.split(",") if v)
    rows = bench_ops(stage_shapes(cfg), args.op_iters, args.reps, sweep)
    lines = ["## gs_attention_kv_* alone (K / V as slices of one buffer; us per call: median (min .. max) of %d "
             "repetitions of %d calls; share of the %.1f TFLOP/s fp32 MFMA peak of the median)"
             % (args.reps, args.op_iters, PEAK_TFLOPS), "",
             "| B | Nq | Nk | heads | forward us | of peak | backward (plan) us | of peak | torch sdpa fwd us | "
             "torch sdpa fwd+bwd us |", "|---|---|---|---|---|---|---|---|---|---|"]
    for (b, nq, nk, heads), us, _, _, _ in rows:
        flops = 4.0 * b * nq * nk * 64 * heads
        f, g = statistics.median(us["fwd"]), statistics.median(us["bwdS"])
        lines.append("| %d | %d | %d | %d | %s | %.1f %% | %s | %.1f %% | %s | %s |" % (
            b, nq, nk, heads, _spread(us["fwd"]), 100 * flops / f * 1e-6 / PEAK_TFLOPS, _spread(us["bwdS"]),
            100 * 2.5 * flops / g * 1e-6 / PEAK_TFLOPS, _spread(us["sdpa_fwd"]), _spread(us["sdpa_fwd_bwd"])))
    lines += ["", "The backward count is the five products of the textbook algorithm (2.5x the forward); the two-"
              "kernel form executes seven.", "",
              "## The query split of the dK / dV kernel: the backward at S = 1 against the plan (alternating; the "
              "delta pre-pass and dQ are the same launches in both)", "",
              "| B | Nq | Nk | heads | planned S | S = 1 us | plan us | plan / S = 1 | spread of S = 1 | plan slower "
              "by more than that spread | workspace S = 1 | workspace plan |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for (b, nq, nk, heads), us, ws1, wsp, planned in rows:
        one, plan = us["bwd1"], us["bwdS"]
        spread = max(one) - min(one)
        lines.append("| %d | %d | %d | %d | %d | %s | %s | x%.3f | %.1f us | %s | %d | %d |" % (
            b, nq, nk, heads, planned, _spread(one), _spread(plan), statistics.median(plan) / statistics.median(one),
            spread, "YES" if statistics.median(plan) - statistics.median(one) > spread else "no", ws1, wsp))
    lines.append("")
    if sweep:
        lines += ["## The backward at forced splits (us, median (min .. max); slabs as clipped to whole tiles)", "",
                  "| B | Nq | Nk | heads | " + " | ".join("S = %d" % s for s in sweep) + " |",
                  "|---|---|---|---|" + "---|" * len(sweep)]
        for (b, nq, nk, heads), us, _, _, _ in rows:
            lines.append("| %d | %d | %d | %d | " % (b, nq, nk, heads) + " | ".join(_spread(us[s]) for s in sweep) + " |")
        lines.append("")
    if not args.skip_steps:
        st = bench_steps(cfg, args)
        lines += ["## Training step of configs/supernet/segformer_mit_b1to3_adamw.py, 1024x512, bs 2 (images/s)", "",
                  "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
                  "| " + " | ".join("%.2f" % v for v in st.values()) + " |", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
