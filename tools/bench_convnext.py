#!/usr/bin/env python
"""The ConvNeXt kernels and the DynamicConvNeXt supernet on the GPU, HIP events
throughout, at 1024x512, bs 2:
  * gs_dwconv2d_* (7x7), gs_layernorm_*, gs_gelu_* and gs_layer_scale_* at the four stage shapes of
    ConvNeXt-T (128x256x96, 64x128x192, 32x64x384, 16x32x768) and of ConvNeXt-B (widths 128 .. 1024),
    forward and backward, each next to torch-ROCm's own operator on the same device and data
    (F.conv2d(groups=C) in channels_last, F.layer_norm, F.gelu, the eager identity + gamma * z), with
    the bytes per second each of our kernels achieves on the bytes its algorithm has to move;
  * the training step (images/s) of configs/supernet/upernet_convnext_t2b.py on the T, S and B anchors
    and on the sampled mix;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout
    and of this one, alternately, each run a process of its own.
Writes its tables to --md (default work_dirs/bench_convnext.md); profiles/r14_convnext.md holds the
tables of one run with the reading of them.

    python tools/bench_convnext.py [--op-iters 50] [--iters 6] [--warmup 2] [--ab-runs 3] [--parent DIR]
                                   [--bench-rounds 3] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_convnext_t2b.py")
STAGES = [(128, 256), (64, 128), (32, 64), (16, 32)]          # 1024x512 input: strides 4, 8, 16, 32
WIDTHS = {"T": (96, 192, 384, 768), "B": (128, 256, 512, 1024)}
EPS = 1e-6


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


def _median_rounds(fns, iters, rounds=3):
    """{name: median us per call} over ``rounds`` interleaved rounds"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(1000 * _time(fn, iters))
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def _torch_bwd(y, inputs, dy):
    return lambda: torch.autograd.grad(y, inputs, dy, retain_graph=True)


def op_cases(n, h, w, c):
    """{operator: ({name: callable}, {name: maps of [n,h,w,width] the algorithm moves}, width)} for one
    stage shape.  GELU runs on the block's hidden width 4c."""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = n * h * w
    rnd = lambda *s: torch.randn(*s, device="cuda")      # noqa: E731
    keep, cases = [], {}
    # depthwise 7x7
    x, dy, y, dx = rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c)
    wt, dwt = rnd(7, 7, 1, c), rnd(7, 7, 1, c)
    d = lib.dwconv_desc(n, h, w, c, 3, 1, k=7)
    db = ctypes.byref(d)
    need = L.gs_dwconv2d_workspace_bytes(db)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    xt = x.permute(0, 3, 1, 2).requires_grad_(True)       # NCHW view of NHWC storage = channels_last
    wtt = wt.permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    yt = F.conv2d(xt, wtt, None, 1, 3, 1, groups=c)
    dyt = dy.permute(0, 3, 1, 2)
    keep += [d, ws]
    cases["dwconv7x7"] = (dict(
        fwd=lambda: lib.check(L.gs_dwconv2d_forward(db, x.data_ptr(), wt.data_ptr(), None, y.data_ptr(), st), "f"),
        dgrad=lambda: lib.check(L.gs_dwconv2d_dgrad(db, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 0, st), "d"),
        wgrad=lambda: lib.check(L.gs_dwconv2d_wgrad(db, x.data_ptr(), dy.data_ptr(), dwt.data_ptr(), ws.data_ptr(),
                                                    need, st), "w"),
        torch_fwd=lambda: F.conv2d(xt, wtt, None, 1, 3, 1, groups=c),
        torch_bwd=_torch_bwd(yt, (xt, wtt), dyt)), dict(fwd=2, dgrad=2, wgrad=2), c)
    # LayerNorm
    g, b, dg, dbs = rnd(c), rnd(c), rnd(c), rnd(c)
    mean, rstd = rnd(rows), rnd(rows)
    ld = lib.layernorm_desc(rows, c, EPS)
    lb = ctypes.byref(ld)
    lneed = L.gs_layernorm_workspace_bytes(lb)
    lws = torch.empty(lneed, dtype=torch.uint8, device="cuda")
    x2 = x.view(rows, c).detach().requires_grad_(True)
    g2, b2 = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y2 = F.layer_norm(x2, (c,), g2, b2, EPS)
    keep += [ld, lws]
    ln_fwd = lambda: lib.check(L.gs_layernorm_forward(lb, x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(),   # noqa: E731
                                                      mean.data_ptr(), rstd.data_ptr(), st), "lf")
    ln_fwd()
    cases["layernorm"] = (dict(
        fwd=ln_fwd,
        bwd=lambda: lib.check(L.gs_layernorm_backward(lb, x.data_ptr(), dy.data_ptr(), g.data_ptr(), mean.data_ptr(),
                                                      rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), dbs.data_ptr(), 0,
                                                      lws.data_ptr(), lneed, st), "lb"),
        torch_fwd=lambda: F.layer_norm(x2, (c,), g2, b2, EPS),
        torch_bwd=_torch_bwd(y2, (x2, g2, b2), dy.view(rows, c))), dict(fwd=2, bwd=3), c)
    # GELU on the hidden width
    c4 = 4 * c
    hx, hdy, hy = rnd(rows, c4), rnd(rows, c4), torch.empty(rows, c4, device="cuda")
    hxt = hx.clone().requires_grad_(True)
    hyt = F.gelu(hxt)
    cases["gelu"] = (dict(
        fwd=lambda: lib.check(L.gs_gelu_forward(hx.data_ptr(), hy.data_ptr(), rows, c4, c4, c4, st), "gf"),
        bwd=lambda: lib.check(L.gs_gelu_backward(hx.data_ptr(), hdy.data_ptr(), hy.data_ptr(), rows, c4, c4, c4, c4,
                                                 st), "gb"),
        torch_fwd=lambda: F.gelu(hxt), torch_bwd=_torch_bwd(hyt, (hxt,), hdy)), dict(fwd=2, bwd=3), c4)
    # layer scale + residual
    sneed = L.gs_layer_scale_workspace_bytes(rows, c)
    sws = torch.empty(sneed, dtype=torch.uint8, device="cuda")
    zt, gt = dx.view(rows, c).detach().clone().requires_grad_(True), g.clone().requires_grad_(True)
    idt = x.view(rows, c).detach()
    ot = idt + gt * zt
    keep += [sws]
    cases["layer_scale_add"] = (dict(
        fwd=lambda: lib.check(L.gs_layer_scale_add_forward(x.data_ptr(), dx.data_ptr(), g.data_ptr(), y.data_ptr(),
                                                           rows, c, c, c, c, st), "sf"),
        bwd=lambda: lib.check(L.gs_layer_scale_backward(dy.data_ptr(), x.data_ptr(), g.data_ptr(), y.data_ptr(),
                                                        dg.data_ptr(), rows, c, c, c, c, sws.data_ptr(), sneed, st),
                              "sb"),
        torch_fwd=lambda: idt + gt * zt, torch_bwd=_torch_bwd(ot, (zt, gt), dy.view(rows, c))),
        dict(fwd=3, bwd=3), c)
    return cases, keep


def bench_ops(iters):
    rows = []
    torch.manual_seed(0)
    for fam, widths in WIDTHS.items():
        for (h, w), c in zip(STAGES, widths):
            cases, keep = op_cases(2, h, w, c)
            for op, (fns, maps, width) in cases.items():
                med = _median_rounds(fns, iters)
                map_bytes = 2 * h * w * width * 4
                ours_bwd = sum(v for k, v in med.items() if k in ("dgrad", "wgrad", "bwd"))
                rows.append(dict(fam=fam, op=op, shape="2x%dx%dx%d" % (h, w, width), med=med,
                                 tbs={k: maps[k] * map_bytes / (med[k] * 1e-6) / 1e12 for k in maps},
                                 fwd_ratio=med["fwd"] / med["torch_fwd"], bwd_ratio=ours_bwd / med["torch_bwd"],
                                 ours_bwd=ours_bwd))
            del cases, keep
            torch.cuda.empty_cache()
    return rows


def _runner(model, sampler_cfg):
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
    hook = ManipulateArchHook(build_model_sampler(sampler_cfg))
    runner.register_hook(hook)
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner, hook


def bench_steps(args):
    """images/s of the training step: one model, the sampler switched between the three anchors and
    the config's train sampler (the mix), interleaved"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    anchors = {m["name"]: m for m in cfg.val_sampler["anchors"]}
    samplers = {k: dict(type="anchor", anchors=[v]) for k, v in anchors.items()}
    samplers["sampled mix"] = cfg.train_sampler
    runner, hook = _runner(model.cuda().train(), samplers["ConvNeXt-T"])
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    out = {k: [] for k in samplers}
    for rnd in range(args.ab_runs + 1):                  # round 0 warms every subnet up
        for k, scfg in samplers.items():
            hook.sampler = build_model_sampler(scfg)
            iters = args.iters * (5 if k == "sampled mix" else 1)
            if rnd == 0:
                _time(lambda: runner.train_iter(batch), max(args.warmup, 5 if k == "sampled mix" else 1), 0)
            else:
                out[k].append(2000.0 / _time(lambda: runner.train_iter(batch), iters, 1))
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
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_convnext.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_convnext.py measures on the GPU: no device found")
    lines = ["## The kernels alone (fp32 NHWC, bs 2; median of 3 interleaved rounds of %d calls, us per call; "
             "TB/s = the bytes the algorithm moves over our kernel's time)" % args.op_iters, "",
             "| op | N x H x W x C | ours fwd | torch fwd | ours / torch | ours bwd | torch bwd | ours / torch | "
             "ours TB/s (per kernel) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in bench_ops(args.op_iters):
        m = r["med"]
        lines.append("| %s (%s) | %s | %.1f | %.1f | %.2f | %.1f | %.1f | %.2f | %s |" % (
            r["op"], r["fam"], r["shape"], m["fwd"], m["torch_fwd"], r["fwd_ratio"], r["ours_bwd"], m["torch_bwd"],
            r["bwd_ratio"], ", ".join("%s %.2f" % kv for kv in r["tbs"].items())))
    lines += ["", "Backward of the depthwise conv = dgrad + wgrad (two launches), of LayerNorm = dx + dweight + "
              "dbias (three launches), of the layer scale = dz + dgamma (two launches); torch's backward "
              "produces the same set of gradients.", ""]
    if not args.skip_steps:
        st = bench_steps(args)
        lines += ["## Training step of configs/supernet/upernet_convnext_t2b.py, 1024x512, bs 2 (interleaved, %d "
                  "runs, images/s)" % args.ab_runs, "", "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
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
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
