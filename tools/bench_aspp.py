#!/usr/bin/env python
"""The DeepLabV3 / DeepLabV3+ heads and their depthwise kernels on the GPU, HIP
events throughout, at 1024x512, bs 2, OS8:
  * gs_dwconv2d_forward / _dgrad / _wgrad at the head's shapes for the R50 and the MAX anchor (the
    three ASPP branches on the 64x128 stage-4 map, the two refinement convs on the 128x256 stage-1
    map), each next to a device-to-device copy of the bytes the kernel has to move;
  * both heads, forward + backward, next to the PSP head on the same stage-4 features;
  * the training step (images/s) of configs/supernet/deeplabv3{,plus}_ar50to101_v1c_os8.py on the R50
    anchor next to pspnet_ar50to101_v1c_os8.py, interleaved;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout
    and of this one, alternately, each run a process of its own.
Writes profiles/r13_aspp_heads.md (--md).

    python tools/bench_aspp.py [--op-iters 50] [--iters 8] [--warmup 3] [--ab-runs 3] [--parent DIR]
                               [--bench-rounds 3] [--skip-steps] [--md profiles/r13_aspp_heads.md]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIGS = {"PSP": "pspnet_ar50to101_v1c_os8.py", "DeepLabV3": "deeplabv3_ar50to101_v1c_os8.py",
           "DeepLabV3+": "deeplabv3plus_ar50to101_v1c_os8.py"}
# stage-4 / stage-1 widths of the anchors (4 x body_width), channels 512, c1_channels 48
ANCHOR_WIDTHS = {"R50": (2048, 256), "MAX": (2560, 320)}


def _time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return b.elapsed_time(e) / iters


def dw_shapes():
    out = []
    for name, (c4, _) in ANCHOR_WIDTHS.items():
        for dil in (12, 24, 36):
            out.append(("%s ASPP branch" % name, 2, 64, 128, c4, dil))
    out.append(("refinement conv 1", 2, 128, 256, 560, 1))
    out.append(("refinement conv 2", 2, 128, 256, 512, 1))
    return out


def bench_dw(iters, rounds=3):
    """us per call of the three kernels and of the copies that move the same bytes: forward and dgrad
    read one map and write one (copy of one map); wgrad reads two maps (copy of two maps' bytes: one
    map copied, 2 x the bytes of reading two)."""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    torch.manual_seed(0)
    for what, n, h, w, c, dil in dw_shapes():
        d = lib.dwconv_desc(n, h, w, c, dil, dil)
        db = ctypes.byref(d)
        x, dy = torch.randn(n, h, w, c, device="cuda"), torch.randn(n, h, w, c, device="cuda")
        y, dx = torch.empty_like(x), torch.empty_like(x)
        wt, dw = torch.randn(3, 3, 1, c, device="cuda"), torch.empty(3, 3, 1, c, device="cuda")
        need = L.gs_dwconv2d_workspace_bytes(db)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        fns = dict(
            fwd=lambda: lib.check(L.gs_dwconv2d_forward(db, x.data_ptr(), wt.data_ptr(), None, y.data_ptr(), st),
                                  "fwd"),
            dgrad=lambda: lib.check(L.gs_dwconv2d_dgrad(db, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 0, st),
                                    "dgrad"),
            wgrad=lambda: lib.check(L.gs_dwconv2d_wgrad(db, x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                                                        ws.data_ptr(), need, st), "wgrad"),
            copy=lambda: y.copy_(x))
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                t[k].append(1000 * _time(fn, iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        rows.append(dict(what=what, shape=(n, h, w, c), dil=dil, map_mb=x.numel() * 4 / 1e6, **med))
    return rows


def anchor(cfg, name):
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:
        if m.get("name") == name:
            m = dict(m)
            if cfg.get("stem_anchors"):   # deep-stem (v1c / OS8) supernet: a width per stem conv (as bench.py)
                m["arch.backbone.stem.width"] = list(cfg["stem_anchors"][name])
            return m
    raise KeyError(name)


def bench_heads(iters, rounds=3):
    """ms of forward + backward (input and parameter gradients) of each head alone on random features
    of the anchor's widths"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_head
    rows = []
    for name, (c4, c1) in ANCHOR_WIDTHS.items():
        torch.manual_seed(0)
        feats = [torch.randn(2, c1, 128, 256, device="cuda"), None, None,
                 torch.randn(2, c4, 64, 128, device="cuda")]
        feats[0] = feats[0].contiguous(memory_format=torch.channels_last).requires_grad_(True)
        feats[3] = feats[3].contiguous(memory_format=torch.channels_last).requires_grad_(True)
        heads, fns = {}, {}
        for label, fname in CONFIGS.items():
            cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", fname))
            heads[label] = build_head(dict(cfg.model["decode_head"], dropout_ratio=0.0)).cuda().train()

            def step(head=heads[label]):
                for p in head.parameters():
                    p.grad = None
                feats[0].grad = feats[3].grad = None
                out = head(feats)
                out.backward(torch.ones_like(out))
            fns[label] = step
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                t[k].append(_time(fn, iters))
        rows.append(dict(anchor=name, **{k: sorted(v)[len(v) // 2] for k, v in t.items()}))
        del heads, fns, feats
        torch.cuda.empty_cache()
    return rows


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
    """images/s of the training step on the R50 anchor, the three configs interleaved"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    runners = {}
    for label, fname in CONFIGS.items():
        cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", fname))
        torch.manual_seed(0)
        model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
        runners[label] = _runner(model.cuda().train(), anchor(cfg, "R50"))
        _time(lambda: runners[label].train_iter(batch), args.warmup, 0)
    out = {k: [] for k in runners}
    for _ in range(args.ab_runs):
        for k, r in runners.items():
            out[k].append(2000.0 / _time(lambda: r.train_iter(batch), args.iters, 1))
    return out


def bench_py_ab(parent, rounds, steps=32, warmup=8):
    """images/s of `bench.py` in ``parent`` and in this checkout, alternately, one process per run."""
    out = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, root in (("parent", parent), ("this", ROOT)):
            res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
                                  "--warmup", str(warmup)], cwd=root, capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError("bench.py failed in %s:\n%s" % (root, res.stderr[-2000:]))
            out[name].append(json.loads(res.stdout.strip().splitlines()[-1])["value"])
            print("bench.py %s: %.2f images/s" % (name, out[name][-1]), flush=True)
    return out


def _runs(v, fmt="%.2f"):
    return "%s (mean %s)" % (" ".join(fmt % x for x in v), fmt % (sum(v) / len(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-heads", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "r13_aspp_heads.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_aspp.py measures on the GPU: no device found")
    lines = ["# DeepLabV3 / DeepLabV3+ heads on the MI355X (tools/bench_aspp.py)", "",
             "## The depthwise kernels alone (fp32 NHWC, pad = dil; median of 3 interleaved rounds of %d calls, "
             "us per call)" % args.op_iters, "",
             "| shape | N, H x W, C | dil | one map MB | forward | dgrad | wgrad (2 launches) | copy of one map | "
             "forward / copy | dgrad / copy | wgrad / copy |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in bench_dw(args.op_iters):
        n, h, w, c = r["shape"]
        lines.append("| %s | %d, %dx%d, %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.2f | %.2f |" % (
            r["what"], n, h, w, c, r["dil"], r["map_mb"], r["fwd"], r["dgrad"], r["wgrad"], r["copy"],
            r["fwd"] / r["copy"], r["dgrad"] / r["copy"], r["wgrad"] / r["copy"]))
    lines += ["", "The copy reads one map and writes one: the bytes the forward and the data gradient have to "
              "move.  The weight gradient reads two maps and writes 9 x C floats per 256 pixels: the same "
              "bytes as the copy.", ""]
    if not args.skip_heads:
        lines += ["## The heads alone, forward + backward on random features, bs 2 (median of 3 interleaved "
                  "rounds of %d, ms)" % args.iters, "", "| anchor widths | " + " | ".join(CONFIGS) + " |",
                  "|---|" + "---|" * len(CONFIGS)]
        for r in bench_heads(args.iters):
            lines.append("| %s | " % r["anchor"] + " | ".join("%.2f" % r[k] for k in CONFIGS) + " |")
        lines.append("")
    if not args.skip_steps:
        st = bench_steps(args)
        lines += ["## Training step on the R50 anchor, 1024x512, bs 2, OS8 (interleaved, %d runs of %d "
                  "iterations, images/s)" % (args.ab_runs, args.iters), "",
                  "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
                  "| " + " | ".join(_runs(v) for v in st.values()) + " |", ""]
    lines += ["## `bench.py --gpus 1 --steps 32 --warmup 8`, parent commit against this commit "
              "(alternating, one process per run, images/s)", ""]
    if ab_py:
        lines += ["| parent | this commit |", "|---|---|",
                  "| %s | %s |" % (_runs(ab_py["parent"]), _runs(ab_py["this"]))]
    else:
        lines += ["Not measured in this run (no --parent checkout given)."]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
