#!/usr/bin/env python
"""The fused GELU + GRN kernels and the DynamicConvNeXtV2 supernet on the GPU, HIP
events throughout, at 1024x512, bs 2:
  * gs_gelu_grn_forward / gs_gelu_grn_backward at the hidden-layer shapes of the four stages of V2-Tiny
    (128x256x384, 64x128x768, 32x64x1536, 16x32x3072) and of V2-Base (widths 512 .. 4096), each next to the
    unfused sequence on what exists without them: gs_gelu_forward, then torch-ROCm's column 2-norm
    (torch.linalg.vector_norm over the pixels) and one torch.addcmul for the apply; backwards, torch's
    autograd of that GRN, then gs_gelu_backward.  us per call, and the GB/s each achieves on the bytes its
    algorithm has to move: three passes over the [N, P, 4C] tensor for the fused forward (x twice, y), five
    for the unfused one (GELU read and write, norm read, apply read and write); five for the fused backward
    (dy and x twice, dx), eight for the unfused one (dy and a for the sums, dy and a and da for the apply,
    da and x and dx for the GELU);
  * the training step (images/s) of configs/supernet/upernet_convnextv2_n2b_adamw.py on its three anchors
    next to the V1 supernet of configs/supernet/upernet_convnext_t2b.py set to the same widths and depths,
    both under the SGD runner of tools/bench_convnext.py, interleaved;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout and of
    this one, alternately, each run a process of its own.
Writes its tables to --md (default work_dirs/bench_convnextv2.md); profiles/r25_convnextv2.md holds the
tables of one run with the reading of them.

    python tools/bench_convnextv2.py [--op-iters 50] [--iters 6] [--warmup 2] [--ab-runs 3] [--parent DIR]
                                     [--bench-rounds 3] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_convnext import STAGES, _runner, _runs, _time, bench_py_ab  # noqa: E402
from gaia_seg_amd.hip import lib  # noqa: E402

CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_convnextv2_n2b_adamw.py")
CONFIG_V1 = os.path.join(ROOT, "configs", "supernet", "upernet_convnext_t2b.py")
WIDTHS = {"V2-Tiny": (96, 192, 384, 768), "V2-Base": (128, 256, 512, 1024)}
EPS = 1e-6
PASSES = dict(fwd=3, unfused_fwd=5, bwd=5, unfused_bwd=8)


def _rounds(fns, iters, rounds=5):
    """{name: (median, min, max) us per call} over ``rounds`` interleaved rounds"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(1000 * _time(fn, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def op_case(n, h, w, c):
    """{name: callable} for the hidden layer [n, h*w, c] of one stage"""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p, rows = h * w, n * h * w
    rnd = lambda *s: torch.randn(*s, device="cuda")      # noqa: E731
    x, dy, y, dx, a = rnd(n, p, c), rnd(n, p, c), rnd(n, p, c), rnd(n, p, c), rnd(n, p, c)
    wt, bs, dwt, dbs, G = rnd(c), rnd(c), rnd(c), rnd(c), rnd(n, c)
    d = lib.gelu_grn_desc(n, p, c, EPS)
    db = ctypes.byref(d)
    need = L.gs_gelu_grn_workspace_bytes(db)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def fwd():
        lib.check(L.gs_gelu_grn_forward(db, x.data_ptr(), wt.data_ptr(), bs.data_ptr(), y.data_ptr(), G.data_ptr(),
                                        ws.data_ptr(), need, st), "grn fwd")

    def bwd():
        lib.check(L.gs_gelu_grn_backward(db, x.data_ptr(), dy.data_ptr(), wt.data_ptr(), G.data_ptr(), dx.data_ptr(),
                                         dwt.data_ptr(), dbs.data_ptr(), ws.data_ptr(), need, st), "grn bwd")

    def grn(t, wv, bv):
        g = torch.linalg.vector_norm(t, ord=2, dim=1, keepdim=True)
        return torch.addcmul(bv, t, 1 + wv * (g / (g.mean(-1, keepdim=True) + EPS)))

    def unfused_fwd():
        lib.check(L.gs_gelu_forward(x.data_ptr(), a.data_ptr(), rows, c, c, c, st), "gelu fwd")
        return grn(a, wt, bs)

    fwd()
    at = a.detach().requires_grad_(True)
    wtt, bst = wt.clone().requires_grad_(True), bs.clone().requires_grad_(True)
    yt = grn(at, wtt, bst)

    def unfused_bwd():
        da = torch.autograd.grad(yt, (at, wtt, bst), dy, retain_graph=True)[0]
        lib.check(L.gs_gelu_backward(x.data_ptr(), da.data_ptr(), dx.data_ptr(), rows, c, c, c, c, st), "gelu bwd")

    return dict(fwd=fwd, unfused_fwd=unfused_fwd, bwd=bwd, unfused_bwd=unfused_bwd), [d, ws, yt]


def bench_ops(iters):
    rows = []
    torch.manual_seed(0)
    for fam, widths in WIDTHS.items():
        for (h, w), c in zip(STAGES, widths):
            fns, keep = op_case(2, h, w, 4 * c)
            stat = _rounds(fns, iters)
            med = {k: v[0] for k, v in stat.items()}
            nbytes = 2 * h * w * 4 * c * 4
            rows.append(dict(fam=fam, shape="2x%dx%dx%d" % (h, w, 4 * c), med=med, mb=nbytes / 1e6,
                             spread=max((v[2] - v[1]) / v[0] for v in stat.values()),
                             gbs={k: PASSES[k] * nbytes / (med[k] * 1e-6) / 1e9 for k in med}))
            del fns, keep
            torch.cuda.empty_cache()
    return rows


def bench_steps(args):
    """images/s of the training step on the three V2 anchors: the V2 supernet and the V1 supernet set to the
    same widths and depths, interleaved"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.synthetic import make_batch
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CONFIG)
    anchors = {m["name"]: m for m in cfg.val_sampler["anchors"]}
    samplers = {k: dict(type="anchor", anchors=[v]) for k, v in anchors.items()}
    first = next(iter(samplers.values()))
    runners = {}
    for tag, path in (("V2", CONFIG), ("V1", CONFIG_V1)):
        c = Config.fromfile(path)
        torch.manual_seed(0)
        model = build_segmentor(c.model, train_cfg=c.get("train_cfg"), test_cfg=c.get("test_cfg"))
        runners[tag] = _runner(model.cuda().train(), first)
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    out = {"%s as %s" % (k, tag): [] for k in samplers for tag in runners}
    for rnd in range(args.ab_runs + 1):                  # round 0 warms every subnet up
        for k, scfg in samplers.items():
            for tag, (runner, hook) in runners.items():
                hook.sampler = build_model_sampler(scfg)
                if rnd == 0:
                    _time(lambda: runner.train_iter(batch), max(args.warmup, 1), 0)
                else:
                    out["%s as %s" % (k, tag)].append(2000.0 / _time(lambda: runner.train_iter(batch), args.iters, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_convnextv2.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_convnextv2.py measures on the GPU: no device found")
    lines = ["## GELU + GRN alone (fp32 NHWC, bs 2; median of 5 interleaved rounds of %d calls; us per call, and "
             "GB/s on %d / %d / %d / %d passes over the tensor)" % (
                 args.op_iters, PASSES["fwd"], PASSES["unfused_fwd"], PASSES["bwd"], PASSES["unfused_bwd"]), "",
             "| net | N x H x W x 4C | MB | fused fwd us (GB/s) | unfused fwd us (GB/s) | unfused / fused | "
             "fused bwd us (GB/s) | unfused bwd us (GB/s) | unfused / fused | widest (max - min) / median |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in bench_ops(args.op_iters):
        m, g = r["med"], r["gbs"]
        lines.append("| %s | %s | %.1f | %.1f (%.0f) | %.1f (%.0f) | %.2f | %.1f (%.0f) | %.1f (%.0f) | %.2f | %.1f%% |" % (
            r["fam"], r["shape"], r["mb"], m["fwd"], g["fwd"], m["unfused_fwd"], g["unfused_fwd"],
            m["unfused_fwd"] / m["fwd"], m["bwd"], g["bwd"], m["unfused_bwd"], g["unfused_bwd"],
            m["unfused_bwd"] / m["bwd"], 100 * r["spread"]))
    lines.append("")
    if not args.skip_steps:
        st = bench_steps(args)
        lines += ["## Training step, 1024x512, bs 2, SGD runner (interleaved, %d runs of %d iterations, images/s): the "
                  "V2 supernet on its anchors, and the V1 supernet at the same widths and depths" % (
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
