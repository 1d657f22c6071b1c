#!/usr/bin/env python
"""The multi-scale convolutional attention kernels and the DynamicMSCAN supernet on the
GPU, HIP events throughout, at 1024x512, bs 2:
  * gs_msca_forward / gs_msca_backward at the four stage shapes of MSCAN-B (2x128x256x64, 2x64x128x128,
    2x32x64x320, 2x16x32x512), each next to the same chain as torch-ROCm computes it: seven depthwise
    F.conv2d calls and three adds, forward and autograd backward (the gradient of the input and of all 14
    parameters), in contiguous NCHW and in channels_last, the faster of the two per shape and direction
    taken as the baseline.  Beside them a device copy of one tensor of the shape (one read, one write): the
    time of a single pass; the table gives each call's time as a multiple of it;  The acceptance figure is the ratio ours / torch of forward plus
    backward summed over the four shapes, which must not exceed 1;
  * gs_gate_mul_forward / _backward at the same shapes next to torch's multiply and its autograd;
  * the training step (images/s) of configs/supernet/upernet_mscan_t2b_adamw.py on its three anchors and on
    the sampled mix, under the config's own AdamW (fused arena kernel, its parameter groups), interleaved;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout and of
    this one, alternately, each run a process of its own.
Writes its tables to --md (default work_dirs/bench_segnext.md); profiles/r26_segnext.md holds the tables of
one run with the reading of them.

    python tools/bench_segnext.py [--op-iters 30] [--iters 6] [--warmup 2] [--ab-runs 3] [--parent DIR]
                                  [--bench-rounds 3] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_convnext import STAGES, _runs, _time, bench_py_ab  # noqa: E402
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_mscan_t2b_adamw.py")
WIDTHS = (64, 128, 320, 512)          # MSCAN-B
K0, KS = 5, (7, 11, 21)
PASSES = dict(fwd=10, bwd=21)         # tensor passes of the fused operator per call (csrc/msca.hip)


def _rounds(fns, iters, rounds=5):
    """{name: (median, min, max) us per call} over ``rounds`` interleaved rounds"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(1000 * _time(fn, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def _torch_chain(x, ps):
    """the chain on an NCHW tensor (any memory format) with OIHW depthwise filters"""
    c = x.shape[1]
    a = F.conv2d(x, ps[0], ps[1], padding=K0 // 2, groups=c)
    s = a
    for i, k in enumerate(KS):
        r = F.conv2d(a, ps[2 + i], ps[5 + i], padding=(0, k // 2), groups=c)
        s = s + F.conv2d(r, ps[8 + i], ps[11 + i], padding=(k // 2, 0), groups=c)
    return s


def msca_case(n, h, w, c):
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rnd = lambda *s: torch.randn(*s, device="cuda")      # noqa: E731
    x, ds, s, dx = rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c)
    shapes = [(K0, K0, c), (c,)] + [(k, c) for k in KS] + [(c,)] * 3 + [(k, c) for k in KS] + [(c,)] * 3
    params = [rnd(*sh) * 0.2 for sh in shapes]
    grads = [torch.empty_like(p) for p in params]
    d = lib.msca_desc(n, h, w, c)
    db = ctypes.byref(d)

    def table(ts):
        p = [t.data_ptr() for t in ts]
        return lib.msca_filters(p[0], p[1], p[2:5], p[5:8], p[8:11], p[11:14])

    f, g = table(params), table(grads)
    saved = torch.empty(L.gs_msca_saved_bytes(db), dtype=torch.uint8, device="cuda")
    need = L.gs_msca_workspace_bytes(db)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def fwd():
        lib.check(L.gs_msca_forward(db, x.data_ptr(), ctypes.byref(f), s.data_ptr(), saved.data_ptr(), st), "msca fwd")

    def bwd():
        lib.check(L.gs_msca_backward(db, x.data_ptr(), ds.data_ptr(), ctypes.byref(f), saved.data_ptr(), dx.data_ptr(),
                                     0, ctypes.byref(g), ws.data_ptr(), need, st), "msca bwd")

    fwd()
    fns = dict(fwd=fwd, bwd=bwd)
    keep = [d, f, g, saved, ws, params, grads]
    # torch: OIHW filters, the input in both memory formats
    oihw = [params[0].permute(2, 0, 1).unsqueeze(1).contiguous(), params[1]]
    oihw += [params[2 + i].t().reshape(c, 1, 1, k).contiguous() for i, k in enumerate(KS)] + params[5:8]
    oihw += [params[8 + i].t().reshape(c, 1, k, 1).contiguous() for i, k in enumerate(KS)] + params[11:14]
    for tag, fmt in (("nchw", torch.contiguous_format), ("nhwc", torch.channels_last)):
        xt = x.permute(0, 3, 1, 2).contiguous(memory_format=fmt).requires_grad_(True)
        dst = ds.permute(0, 3, 1, 2).contiguous(memory_format=fmt)
        pt = [p.detach().clone().requires_grad_(True) for p in oihw]
        yt = _torch_chain(xt, pt)

        def t_fwd(xt=xt, pt=pt):
            with torch.no_grad():
                return _torch_chain(xt, pt)

        def t_bwd(yt=yt, xt=xt, pt=pt, dst=dst):
            return torch.autograd.grad(yt, [xt] + pt, dst, retain_graph=True)

        fns["torch_fwd_" + tag], fns["torch_bwd_" + tag] = t_fwd, t_bwd
        keep += [xt, dst, pt, yt]
    cp = torch.empty_like(x)
    fns["copy"] = lambda: cp.copy_(x)
    # gate
    gq, u, y, dg, du = rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c), rnd(n, h, w, c)
    rows = n * h * w

    def gate_fwd():
        lib.check(L.gs_gate_mul_forward(gq.data_ptr(), u.data_ptr(), y.data_ptr(), rows, c, c, c, c, st), "gate fwd")

    def gate_bwd():
        lib.check(L.gs_gate_mul_backward(ds.data_ptr(), gq.data_ptr(), u.data_ptr(), dg.data_ptr(), du.data_ptr(), rows,
                                         c, c, c, c, c, c, 1, st), "gate bwd")

    gt, ut = gq.clone().requires_grad_(True), u.clone().requires_grad_(True)
    yt2 = gt * ut
    fns.update(gate_fwd=gate_fwd, gate_bwd=gate_bwd, torch_gate_fwd=lambda: torch.mul(gq, u),
               torch_gate_bwd=lambda: torch.autograd.grad(yt2, (gt, ut), ds, retain_graph=True))
    keep += [cp, gq, u, y, dg, du, gt, ut, yt2]
    return fns, keep


def bench_ops(iters):
    rows = []
    torch.manual_seed(0)
    for (h, w), c in zip(STAGES, WIDTHS):
        fns, keep = msca_case(2, h, w, c)
        stat = _rounds(fns, iters)
        med = {k: v[0] for k, v in stat.items()}
        rows.append(dict(shape="2x%dx%dx%d" % (h, w, c), med=med, mb=2 * h * w * c * 4 / 1e6,
                         spread=max((v[2] - v[1]) / v[0] for v in stat.values())))
        del fns, keep
        torch.cuda.empty_cache()
    return rows


def _adamw_runner(model, cfg, sampler_cfg):
    """the config's own optimizer: AdamW on the fused arena kernel with its parameter groups, at a fixed
    learning rate (the schedule's warm-up would scale the measured steps to nothing)"""
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner,
                                          ManipulateArchHook)
    opt = check_optimizer_cfg(cfg.optimizer)
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             param_groups=build_param_groups(model, cfg.optimizer))
    hook = ManipulateArchHook(build_model_sampler(sampler_cfg))
    runner.register_hook(hook)
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner, hook


def bench_steps(args):
    """images/s of the training step under the config's AdamW: one model, the sampler switched between the
    three anchors and the config's train sampler (the mix), interleaved"""
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
    runner, hook = _adamw_runner(model.cuda().train(), cfg, samplers["MIN"])
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    out = {k: [] for k in samplers}
    for rnd in range(args.ab_runs + 1):                  # round 0 warms every subnet up
        for k, scfg in samplers.items():
            hook.sampler = build_model_sampler(scfg)
            iters = args.iters * (3 if k == "sampled mix" else 1)
            if rnd == 0:
                _time(lambda: runner.train_iter(batch), max(args.warmup, 3 if k == "sampled mix" else 1), 0)
            else:
                out[k].append(2000.0 / _time(lambda: runner.train_iter(batch), iters, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=30)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_segnext.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_segnext.py measures on the GPU: no device found")
    rows = bench_ops(args.op_iters)
    lines = ["## gs_msca_* alone (fp32, bs 2; median of 5 interleaved rounds of %d calls; us per call; GB/s on the "
             "%d / %d tensor passes of the fused forward / backward; torch = the faster of NCHW and channels_last)"
             % (args.op_iters, PASSES["fwd"], PASSES["bwd"]), "",
             "| N x H x W x C | MB | copy us | ours fwd us (GB/s) | in copies | torch fwd nchw / nhwc us | "
             "ours / torch | ours bwd us (GB/s) | in copies | torch bwd nchw / nhwc us | ours / torch | "
             "fwd + bwd ours / torch | widest (max - min) / median |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    tot_o = tot_t = 0.0
    for r in rows:
        m = r["med"]
        tf, tb = min(m["torch_fwd_nchw"], m["torch_fwd_nhwc"]), min(m["torch_bwd_nchw"], m["torch_bwd_nhwc"])
        tot_o += m["fwd"] + m["bwd"]
        tot_t += tf + tb
        gbs = lambda k: PASSES[k] * r["mb"] * 1e6 / (m[k] * 1e-6) / 1e9      # noqa: E731
        lines.append("| %s | %.1f | %.1f | %.1f (%.0f) | %.1f | %.1f / %.1f | %.2f | %.1f (%.0f) | %.1f | %.1f / %.1f | "
                     "%.2f | %.2f | %.1f%% |" % (
                         r["shape"], r["mb"], m["copy"], m["fwd"], gbs("fwd"), m["fwd"] / m["copy"],
                         m["torch_fwd_nchw"], m["torch_fwd_nhwc"], m["fwd"] / tf, m["bwd"], gbs("bwd"),
                         m["bwd"] / m["copy"], m["torch_bwd_nchw"], m["torch_bwd_nhwc"], m["bwd"] / tb,
                         (m["fwd"] + m["bwd"]) / (tf + tb), 100 * r["spread"]))
    lines += ["", "Summed over the four shapes, forward plus backward: ours %.1f us, torch %.1f us, ours / torch = "
              "**%.3f** (acceptance: at most 1)." % (tot_o, tot_t, tot_o / tot_t), "",
              "## gs_gate_mul_* alone (same protocol; us per call)", "",
              "| N x H x W x C | ours fwd | torch fwd | ours / torch | ours bwd | torch bwd | ours / torch |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        m = r["med"]
        lines.append("| %s | %.1f | %.1f | %.2f | %.1f | %.1f | %.2f |" % (
            r["shape"], m["gate_fwd"], m["torch_gate_fwd"], m["gate_fwd"] / m["torch_gate_fwd"], m["gate_bwd"],
            m["torch_gate_bwd"], m["gate_bwd"] / m["torch_gate_bwd"]))
    lines.append("")
    if not args.skip_steps:
        st = bench_steps(args)
        lines += ["## Training step, 1024x512, bs 2, the config's AdamW (interleaved, %d runs of %d iterations, images/s)" % (
            args.ab_runs, args.iters), "", "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
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
