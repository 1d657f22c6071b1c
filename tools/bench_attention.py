#!/usr/bin/env python
"""The attention operator and the elastic ViT supernet on the GPU, HIP events
throughout, at 1024x512 (N = 2049 tokens), bs 2:
  * gs_attention_forward / gs_attention_backward and their fp16-operand twins (gs_attention_*_f16, DESIGN.md
    section 32) per (B, N, heads) of the anchors of configs/supernet/upernet_elastic_vit.py (Q, K, V as three
    column slices of one buffer, as the backbone lays them out), the two precisions alternating over --reps
    repetitions, with the TFLOP/s of the 4 * N^2 * 64 * heads forward and 2.5x that backward count;
  * the training step (images/s) of that config on its MIN and MAX anchors;
  * --fp16-steps: the training step of upernet_elastic_vit_adamw_fp16.py (AdamW, Fp16OptimizerHook) on MIN and
    MAX with fp16_attention off and on, alternating.
Writes its tables to --md (default work_dirs/bench_attention.md); profiles/r15_attention.md and
profiles/r19_fp16_attention.md say which of them have been measured.

    python tools/bench_attention.py [--op-iters 20] [--reps 5] [--iters 4] [--warmup 2] [--skip-steps]
                                    [--fp16-steps] [--md FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit.py")


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


def anchors():
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(CONFIG)
    return cfg, {m["name"]: m for m in cfg.val_sampler["anchors"]}


def bench_ops(cfg, metas, iters, reps):
    """[(anchor, B, N, heads, {(entry, precision): [ms per repetition]})]: one row per distinct head count of
    an anchor; entry 'fwd' / 'bwd', precision 'fp32' / 'fp16' (gs_attention_*_f16), the two precisions
    alternating inside every repetition"""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    h, w = cfg.model["backbone"]["img_size"]
    patch = cfg.model["backbone"]["patch_size"]
    b, n = cfg.data["samples_per_gpu"], 1 + (h // patch) * (w // patch)
    rows, seen = [], set()
    for name, meta in metas.items():
        for heads in meta["arch.backbone.encoder.num_heads.num_heads.num_heads"]:
            if heads in seen:
                continue
            seen.add(heads)
            c = 64 * heads
            qkv, dqkv = torch.randn(b, n, 3 * c, device="cuda"), torch.empty(b, n, 3 * c, device="cuda")
            o, do = torch.empty(b, n, c, device="cuda"), torch.randn(b, n, c, device="cuda")
            lse = torch.empty(b * heads * n, device="cuda")
            d = lib.attention_desc(b, n, heads, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c)
            db = ctypes.byref(d)
            need = max(L.gs_attention_workspace_bytes(db), L.gs_attention_workspace_bytes_f16(db))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            p, g = qkv.data_ptr(), dqkv.data_ptr()

            def fwd(sfx):
                lib.check(getattr(L, "gs_attention_forward" + sfx)(db, p, p + 4 * c, p + 8 * c, o.data_ptr(),
                                                                   lse.data_ptr(), st), "fwd" + sfx)

            def bwd(sfx):
                lib.check(getattr(L, "gs_attention_backward" + sfx)(
                    db, p, p + 4 * c, p + 8 * c, o.data_ptr(), lse.data_ptr(), do.data_ptr(), g, g + 4 * c,
                    g + 8 * c, 0, ws.data_ptr(), need, st), "bwd" + sfx)

            ms = {(e, pr): [] for e in ("fwd", "bwd") for pr in ("fp32", "fp16")}
            for _ in range(reps):
                for pr, sfx in (("fp32", ""), ("fp16", "_f16")):
                    fwd(sfx)    # (the backward reads the O and lse of its own forward)
                    ms[("fwd", pr)].append(_time(lambda: fwd(sfx), iters))
                    ms[("bwd", pr)].append(_time(lambda: bwd(sfx), iters))
            rows.append((name, b, n, heads, ms))
    return rows


def bench_fp16_steps(args):
    """{anchor: {flag: [images/s per repetition]}} of configs/supernet/upernet_elastic_vit_adamw.py under
    Fp16OptimizerHook(loss_scale=512.), fp16_attention off and on alternating on one runner"""
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, IterBasedRunner
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG.replace(".py", "_adamw_fp16.py"))
    metas = {m["name"]: m for m in cfg.val_sampler["anchors"]}
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    opt = check_optimizer_cfg(cfg.optimizer)
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             param_groups=build_param_groups(model, cfg.optimizer))
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(optimizer_hook(cfg.optimizer_config, cfg.fp16))
    runner.call_hook("before_run")
    assert model.backbone.fp16_attention and runner.train_precision == "fp16"
    h, w = cfg.model["backbone"]["img_size"]
    bs = cfg.data["samples_per_gpu"]
    batch = make_batch(bs, h, w, seed=0, device="cuda")
    out = {}
    for name in ("MIN", "MAX"):
        runner.set_arch(metas[name])
        out[name] = {False: [], True: []}
        for _ in range(args.reps):
            for flag in (False, True):
                model.backbone.fp16_attention = flag
                out[name][flag].append(1000.0 * bs / _time(lambda: runner.train_iter(batch), args.iters, args.warmup))
    return out


def _spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def bench_steps(cfg, metas, args):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.01,
                             momentum=0.9, weight_decay=5e-4, max_iters=10 ** 6)
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    h, w = cfg.model["backbone"]["img_size"]
    bs = cfg.data["samples_per_gpu"]
    batch = make_batch(bs, h, w, seed=0, device="cuda")
    out = {}
    for name in ("MIN", "MAX"):
        runner.set_arch(metas[name])
        out[name] = 1000.0 * bs / _time(lambda: runner.train_iter(batch), args.iters, args.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--fp16-steps", action="store_true")
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_attention.md"))
    args = ap.parse_args()
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_attention.py measures on the GPU: no device found")
    cfg, metas = anchors()
    lines = ["## gs_attention_* and gs_attention_*_f16 alone (Q / K / V as slices of one buffer; ms per call: "
             "median (min .. max) of %d repetitions of %d calls, fp32 and fp16 alternating)" % (args.reps, args.op_iters),
             "", "| anchor | B | N | heads | entry | fp32 ms | fp32 TFLOP/s | fp16 ms | fp16 TFLOP/s | speed-up | "
             "faster by more than the spread |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, b, n, heads, ms in bench_ops(cfg, metas, args.op_iters, args.reps):
        for entry, mult in (("fwd", 1.0), ("bwd", 2.5)):
            flops = mult * 4.0 * b * n * n * 64 * heads
            a, f = ms[(entry, "fp32")], ms[(entry, "fp16")]
            lines.append("| %s | %d | %d | %d | %s | %s | %.1f | %s | %.1f | x%.2f | %s |" % (
                name, b, n, heads, entry, _spread(a), flops / statistics.median(a) * 1e-9, _spread(f),
                flops / statistics.median(f) * 1e-9, statistics.median(a) / statistics.median(f),
                "yes" if max(f) < min(a) else "NO"))
    lines += ["", "The backward count is the five products of the textbook algorithm (2.5x the forward); the two-"
              "kernel form executes seven.", ""]
    if not args.skip_steps:
        st = bench_steps(cfg, metas, args)
        lines += ["## Training step of configs/supernet/upernet_elastic_vit.py, 1024x512, bs 2 (images/s)", "",
                  "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
                  "| " + " | ".join("%.2f" % v for v in st.values()) + " |", ""]
    if args.fp16_steps:
        lines += ["## Training step of configs/supernet/upernet_elastic_vit_adamw_fp16.py, 1024x512, bs 2 (images/s: "
                  "median (min .. max) of %d repetitions, fp16_attention off and on alternating)" % args.reps, "",
                  "| anchor | Fp16OptimizerHook | + fp16.attention | speed-up |", "|---|---|---|---|"]
        for name, res in bench_fp16_steps(args).items():
            lines.append("| %s | %s | %s | x%.3f |" % (name, _spread(res[False]), _spread(res[True]),
                                                      statistics.median(res[True]) / statistics.median(res[False])))
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
