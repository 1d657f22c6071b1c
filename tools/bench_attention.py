#!/usr/bin/env python
"""The attention operator and the elastic ViT supernet on the GPU, HIP events
throughout, at 1024x512 (N = 2049 tokens), bs 2:
  * gs_attention_forward / gs_attention_backward per (B, N, heads) of the anchors of
    configs/supernet/upernet_elastic_vit.py (Q, K, V as three column slices of one buffer, as the backbone
    lays them out), with the TFLOP/s of the 4 * N^2 * 64 * heads forward and 2.5x that backward count;
  * the training step (images/s) of that config on its MIN and MAX anchors.
Writes its tables to --md (default work_dirs/bench_attention.md); profiles/r15_attention.md says which of
them have been measured.

    python tools/bench_attention.py [--op-iters 20] [--iters 4] [--warmup 2] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import os
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


def bench_ops(cfg, metas, iters):
    """[(anchor, B, N, heads, forward ms, backward ms)]: one row per distinct head count of an anchor"""
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
            need = L.gs_attention_workspace_bytes(db)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            p, g = qkv.data_ptr(), dqkv.data_ptr()
            fwd = lambda: lib.check(L.gs_attention_forward(db, p, p + 4 * c, p + 8 * c, o.data_ptr(),   # noqa: E731
                                                           lse.data_ptr(), st), "fwd")
            bwd = lambda: lib.check(L.gs_attention_backward(db, p, p + 4 * c, p + 8 * c, o.data_ptr(),   # noqa: E731
                                                            lse.data_ptr(), do.data_ptr(), g, g + 4 * c, g + 8 * c, 0,
                                                            ws.data_ptr(), need, st), "bwd")
            rows.append((name, b, n, heads, _time(fwd, iters), _time(bwd, iters)))
    return rows


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
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_attention.md"))
    args = ap.parse_args()
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_attention.py measures on the GPU: no device found")
    cfg, metas = anchors()
    lines = ["## gs_attention_* alone (fp32, Q / K / V as slices of one buffer; %d calls, ms per call)" % args.op_iters,
             "", "| anchor | B | N | heads | forward ms | TFLOP/s | backward ms | TFLOP/s |", "|---|---|---|---|---|---|---|---|"]
    for name, b, n, heads, tf, tb in bench_ops(cfg, metas, args.op_iters):
        flops = 4.0 * b * n * n * 64 * heads
        lines.append("| %s | %d | %d | %d | %.3f | %.1f | %.3f | %.1f |" % (
            name, b, n, heads, tf, flops / tf * 1e-9, tb, 2.5 * flops / tb * 1e-9))
    lines += ["", "The backward count is the five products of the textbook algorithm (2.5x the forward); the two-"
              "kernel form executes seven.", ""]
    if not args.skip_steps:
        st = bench_steps(cfg, metas, args)
        lines += ["## Training step of configs/supernet/upernet_elastic_vit.py, 1024x512, bs 2 (images/s)", "",
                  "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
                  "| " + " | ".join("%.2f" % v for v in st.values()) + " |", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
