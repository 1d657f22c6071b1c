#!/usr/bin/env python
"""The ElasticConvformer coupling kernels and supernet on the GPU, HIP events
throughout, at 1024x512, bs 2 (2048 tokens + cls per image), at the shapes of the MIN and MAX anchors of
configs/_dynamic_/model_samplers/elastic_convformer.py:
  * gs_fcu_down_forward / _backward next to the composition of existing entries it replaces: gs_layernorm_*,
    gs_gelu_*, one gs_copy2d per image for the token rows and one for the cls row, and the two gs_copy2d of
    the residual add (backward: the copies in reverse, gs_gelu_backward, gs_layernorm_backward);
  * gs_fcu_up_add_forward / _backward next to two gs_copy2d (copy, then add) at s = 1; the library has no
    nearest upsample to compose at s > 1, so there the neighbour is torch-ROCm's F.interpolate + add in
    channels_last, and autograd's backward of it;
  * the training step (images/s) of configs/supernet/upernet_elastic_convformer_adamw.py on the MIN and MAX
    anchors.
Fused kernels and their neighbours are timed alternately in the same process, five repetitions; the table
gives the median and the spread (min .. max) of each and the ratio of the medians.
Writes its tables to --md (default work_dirs/bench_convformer.md); profiles/r20_convformer.md holds the
tables of one run with the reading of them.

    python tools/bench_convformer.py [--op-iters 50] [--reps 5] [--iters 6] [--warmup 2] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_convformer_adamw.py")
B, TOKENS = 2, 32 * 64
EMBED = {"MIN": 384, "MAX": 576}
# (H, W, s) of the 3x3 conv's input in stages 1, 2, 3 (stage 4 repeats stage 3's); C = width / 4
UP_STAGES = [(128, 256, 4), (64, 128, 2), (32, 64, 1)]
WIDTHS = {"MIN": (256, 512, 1024), "MAX": (384, 768, 1536)}
EPS = 1e-5


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


def _alternate(fns, iters, reps):
    """{name: sorted us per call over ``reps`` repetitions}, the callables taking turns"""
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(1000 * _time(fn, iters))
    return {k: sorted(v) for k, v in t.items()}


def down_case(d):
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rnd = lambda *s: torch.randn(*s, device="cuda")      # noqa: E731
    t, n = TOKENS, TOKENS + 1
    z, xt, dout = rnd(B * t, d), rnd(B * n, d), rnd(B * n, d)
    out, dz, dxt = rnd(B * n, d), rnd(B * t, d), rnd(B * n, d)
    t1, t2, dt2 = rnd(B * t, d), rnd(B * t, d), rnd(B * t, d)
    g, b, dg, db_ = rnd(d), rnd(d), rnd(d), rnd(d)
    mean, rstd = rnd(B * t), rnd(B * t)
    fd = lib.fcu_down_desc(B, t, d, EPS)
    fb = ctypes.byref(fd)
    fneed = L.gs_fcu_down_workspace_bytes(fb)
    ld = lib.layernorm_desc(B * t, d, EPS)
    lb = ctypes.byref(ld)
    lneed = L.gs_layernorm_workspace_bytes(lb)
    ws = torch.empty(max(fneed, lneed), dtype=torch.uint8, device="cuda")
    ck = lib.check

    def copy(src, s0, dst, d0, rows, scale=1.0, acc=0):
        ck(L.gs_copy2d(src.data_ptr() + 4 * s0 * d, d, dst.data_ptr() + 4 * d0 * d, d, rows, d, scale, acc, st), "c")

    def fused_fwd():
        ck(L.gs_fcu_down_forward(fb, z.data_ptr(), xt.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(),
                                 mean.data_ptr(), rstd.data_ptr(), st), "ff")

    def fused_bwd():
        ck(L.gs_fcu_down_backward(fb, z.data_ptr(), dout.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), dz.data_ptr(), dxt.data_ptr(), dg.data_ptr(), db_.data_ptr(), 0,
                                  ws.data_ptr(), fneed, st), "fb")

    def composed_fwd():
        ck(L.gs_layernorm_forward(lb, z.data_ptr(), g.data_ptr(), b.data_ptr(), t1.data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), st), "lf")
        ck(L.gs_gelu_forward(t1.data_ptr(), t2.data_ptr(), B * t, d, d, d, st), "gf")
        for i in range(B):
            copy(t2, i * t, dxt, i * n + 1, t)          # (dxt: the [B, T + 1, D] staging buffer)
            copy(xt, i * n, dxt, i * n, 1)
        copy(dxt, 0, out, 0, B * n)
        copy(xt, 0, out, 0, B * n, acc=1)

    def composed_bwd():
        copy(dout, 0, dxt, 0, B * n)
        for i in range(B):
            copy(dout, i * n, dxt, i * n, 1, acc=1)
            copy(dout, i * n + 1, dt2, i * t, t)
        ck(L.gs_gelu_backward(t1.data_ptr(), dt2.data_ptr(), dt2.data_ptr(), B * t, d, d, d, d, st), "gb")
        ck(L.gs_layernorm_backward(lb, z.data_ptr(), dt2.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                   dz.data_ptr(), dg.data_ptr(), db_.data_ptr(), 0, ws.data_ptr(), lneed, st), "lb")

    composed_fwd()
    keep = [fd, ld, ws]
    return dict(fused_fwd=fused_fwd, composed_fwd=composed_fwd, fused_bwd=fused_bwd, composed_bwd=composed_bwd), keep


def up_case(h, w, c, s):
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rnd = lambda *sh: torch.randn(*sh, device="cuda")      # noqa: E731
    x, dout, out = rnd(B, h, w, c), rnd(B, h, w, c), rnd(B, h, w, c)
    r, dr = rnd(B, h // s, w // s, c), rnd(B, h // s, w // s, c)
    rows = B * h * w
    ck = lib.check
    fns = dict(
        fused_fwd=lambda: ck(L.gs_fcu_up_add_forward(x.data_ptr(), r.data_ptr(), out.data_ptr(), B, h, w, c, s, c, c,
                                                     c, st), "uf"),
        fused_bwd=lambda: ck(L.gs_fcu_up_add_backward(dout.data_ptr(), dr.data_ptr(), B, h, w, c, s, c, c, 0, st),
                             "ub"))
    if s == 1:
        def composed_fwd():
            ck(L.gs_copy2d(x.data_ptr(), c, out.data_ptr(), c, rows, c, 1.0, 0, st), "c")
            ck(L.gs_copy2d(r.data_ptr(), c, out.data_ptr(), c, rows, c, 1.0, 1, st), "c")
        fns["composed_fwd"] = composed_fwd
        fns["composed_bwd"] = lambda: ck(L.gs_copy2d(dout.data_ptr(), c, dr.data_ptr(), c, rows, c, 1.0, 0, st), "c")
    else:
        xt = x.permute(0, 3, 1, 2)
        rt = r.permute(0, 3, 1, 2).requires_grad_(True)
        yt = xt + F.interpolate(rt, size=(h, w))
        dyt = dout.permute(0, 3, 1, 2)
        fns["composed_fwd"] = lambda: xt + F.interpolate(rt, size=(h, w))
        fns["composed_bwd"] = lambda: torch.autograd.grad(yt, (rt,), dyt, retain_graph=True)
    return fns, [x, dout, out, r, dr]


def bench_ops(iters, reps):
    rows = []
    torch.manual_seed(0)
    for fam in ("MIN", "MAX"):
        cases = [("fcu_down", "%dx%dx%d" % (B, TOKENS, EMBED[fam]), "existing entries") + down_case(EMBED[fam])]
        for (h, w, s), width in zip(UP_STAGES, WIDTHS[fam]):
            cases.append(("fcu_up_add", "%dx%dx%dx%d s=%d" % (B, h, w, width // 4, s),
                          "two gs_copy2d" if s == 1 else "torch interpolate + add") + up_case(h, w, width // 4, s))
        for op, shape, neighbour, fns, keep in cases:
            t = _alternate(fns, iters, reps)
            rows.append(dict(fam=fam, op=op, shape=shape, neighbour=neighbour, t=t))
            del fns, keep
        torch.cuda.empty_cache()
    return rows


def bench_steps(args):
    """images/s of the training step on the MIN and MAX anchors: one model, the config's AdamW, the two
    subnets taking turns"""
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner, ManipulateArchHook
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    torch.manual_seed(0)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    opt = check_optimizer_cfg(cfg.optimizer)
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=10 ** 6,
                             param_groups=build_param_groups(model, cfg.optimizer))
    anchors = {m["name"]: m for m in cfg.val_sampler["anchors"]}
    samplers = {k: dict(type="anchor", anchors=[anchors[k]]) for k in ("MIN", "MAX")}
    hook = ManipulateArchHook(build_model_sampler(samplers["MIN"]))
    runner.register_hook(hook)
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    batch = make_batch(B, 512, 1024, seed=0, device="cuda")
    out = {k: [] for k in samplers}
    for rnd in range(args.reps + 1):                  # round 0 warms both subnets up
        for k, scfg in samplers.items():
            hook.sampler = build_model_sampler(scfg)
            if rnd == 0:
                _time(lambda: runner.train_iter(batch), max(args.warmup, 1), 0)
            else:
                out[k].append(1000.0 * B / _time(lambda: runner.train_iter(batch), args.iters, 1))
    return out


def _spread(v, fmt="%.1f"):
    return "%s (%s .. %s)" % (fmt % v[len(v) // 2], fmt % v[0], fmt % v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_convformer.md"))
    args = ap.parse_args()
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_convformer.py measures on the GPU: no device found")
    lines = ["## The coupling kernels alone (fp32, bs 2; %d alternating repetitions of %d calls; us per call: median "
             "(min .. max); ratio = fused median / neighbour median)" % (args.reps, args.op_iters), "",
             "| op | shape | neighbour | fused fwd | neighbour fwd | ratio | outside the spread | fused bwd | "
             "neighbour bwd | ratio | outside the spread |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in bench_ops(args.op_iters, args.reps):
        t = r["t"]
        cells = []
        for d in ("fwd", "bwd"):
            f, c = t["fused_" + d], t["composed_" + d]
            cells += [_spread(f), _spread(c), "%.2f" % (f[len(f) // 2] / c[len(c) // 2]),
                      "yes" if (f[-1] < c[0] or c[-1] < f[0]) else "NO"]
        lines.append("| %s (%s) | %s | %s | %s |" % (r["op"], r["fam"], r["shape"], r["neighbour"], " | ".join(cells)))
    lines += ["", "'outside the spread': the two sets of repetitions do not overlap.", ""]
    if not args.skip_steps:
        st = bench_steps(args)
        lines += ["## Training step of configs/supernet/upernet_elastic_convformer_adamw.py, 1024x512, bs 2 "
                  "(alternating, %d repetitions of %d steps, images/s: median (min .. max))" % (args.reps, args.iters),
                  "", "| " + " | ".join(st) + " |", "|" + "---|" * len(st),
                  "| " + " | ".join(_spread(sorted(v), "%.2f") for v in st.values()) + " |", ""]
    else:
        lines += ["## Training step", "", "Not measured in this run (--skip-steps).", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
