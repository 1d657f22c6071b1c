#!/usr/bin/env python
"""OCRNet's two region operators, its head and its recipe on the GPU, HIP events
throughout, at the recipe shape: bs 2, a 64x128 stride-8 map of a 512x1024 crop, K = 19 classes, C = 512
feature channels, ch = 256 attention channels.
  * every C-ABI call of csrc/ocr.hip (gather forward / backward, attend forward / backward) timed by an event
    pair per call, next to the bytes it has to move (inputs read once, outputs written once) and to
    gs_copy2d moving that many bytes in the same run;
  * with --kernel-stats CSV (the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of
    `tools/bench_ocr.py --loop-ops N`, a run of its own) the same per kernel;
  * each operator next to its torch composition (softmax + bmm with autograd) in the same process;
  * DynamicOCRHead forward + backward next to DynamicASPPHead on the same stage-4 features;
  * the training step (images/s) of configs/supernet/ocrnet_ar50to101_v1c_os8.py on the R50 anchor next to
    deeplabv3_ar50to101_v1c_os8.py, interleaved;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout and of
    this one, alternately, each run a process of its own.
Writes profiles/r22_ocr_head.md (--md).

    python tools/bench_ocr.py [--op-iters 50] [--iters 8] [--warmup 3] [--ab-runs 3] [--parent DIR]
                              [--bench-rounds 3] [--skip-steps] [--skip-heads] [--kernel-stats CSV]
                              [--loop-ops N] [--md profiles/r22_ocr_head.md]"""
import argparse
import csv
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaia_seg_amd.hip import lib  # noqa: E402
from bench_aspp import _runner, _runs, _time, anchor, bench_py_ab  # noqa: E402

B, H, W, K, C, CH = 2, 64, 128, 19, 512, 256
P, KP = H * W, 20
CONFIGS = {"DeepLabV3": "deeplabv3_ar50to101_v1c_os8.py", "OCRNet": "ocrnet_ar50to101_v1c_os8.py"}
F4 = 4  # bytes per float


def kernel_bytes():
    """bytes every kernel has to move at the recipe shape: inputs read once, outputs written once.  Keys are
    substrings of the kernels' names; (call, kernel, launches per forward + backward, bytes of all of them)."""
    runs = (P + 127) // 128
    part_c, part_ch = B * runs * K * C * F4, B * runs * K * CH * F4
    return [
        ("gather fwd", "ocr_stats_partial_kernel", 1, B * P * K * F4),
        ("gather fwd", "ocr_stats_final_kernel", 1, 0),
        ("gather fwd", "ocr_prod_partial_kernel<true>", 1, B * P * (C + K) * F4 + part_c),
        ("gather bwd", "ocr_gather_t_kernel", 1, 2 * B * K * C * F4),
        ("gather bwd", "ocr_gather_bwd_kernel", 1, B * P * (2 * C + 2 * K) * F4 + B * K * C * F4),
        ("attend fwd", "ocr_attend_fwd_kernel", 1, B * P * (2 * CH + 1) * F4 + 2 * B * K * CH * F4),
        ("attend bwd", "ocr_attend_bwd_kernel", 1, B * P * (4 * CH + 1 + 2 * K) * F4 + 2 * B * K * CH * F4),
        ("attend bwd", "ocr_prod_partial_kernel<false>", 2, 2 * (B * P * (CH + K) * F4 + part_ch)),
        # one name for the [K x C] sum of the gather and the two [K x ch] sums of the attend backward
        ("gather fwd, attend bwd", "ocr_prod_sum_kernel", 3,
         part_c + B * K * C * F4 + 2 * (part_ch + B * K * CH * F4)),
    ]


def call_bytes():
    runs = (P + 127) // 128
    out = {}
    for call, name, _, n in kernel_bytes():
        if name != "ocr_prod_sum_kernel":
            out[call] = out.get(call, 0) + n
    out["gather fwd"] += B * runs * K * C * F4 + B * K * C * F4
    out["attend bwd"] += 2 * (B * runs * K * CH * F4 + B * K * CH * F4)
    return out


class Ops:
    """the four C-ABI calls on device buffers of the recipe shape"""

    def __init__(self):
        self.L = L = lib.load()
        g = torch.Generator(device="cuda").manual_seed(0)

        def rnd(*s):
            return torch.randn(*s, device="cuda", generator=g)
        self.logits = torch.zeros(B, P, KP, device="cuda")
        self.logits[..., :K] = 3.0 * rnd(B, P, K)
        self.feats, self.dctx = rnd(B, P, C), rnd(B, K, C)
        self.q, self.k, self.v, self.dout = rnd(B, P, CH), rnd(B, K, CH), rnd(B, K, CH), rnd(B, P, CH)
        self.ctx, self.stats = torch.empty(B, K, C, device="cuda"), torch.empty(B, K, 2, device="cuda")
        self.dl, self.df = torch.empty(B, P, KP, device="cuda"), torch.empty(B, P, C, device="cuda")
        self.out, self.lse = torch.empty(B, P, CH, device="cuda"), torch.empty(B, P, device="cuda")
        self.dq, self.dk, self.dv = (torch.empty_like(t) for t in (self.q, self.k, self.v))
        self.gd, self.ad = lib.ocr_gather_desc(B, P, K, C, 1.0), lib.ocr_attend_desc(B, P, K, CH)
        need = max(L.gs_ocr_gather_workspace_bytes(ctypes.byref(self.gd)),
                   L.gs_ocr_attend_workspace_bytes(ctypes.byref(self.ad)))
        self.ws, self.need = torch.empty(need, dtype=torch.uint8, device="cuda"), need
        self.st = torch.cuda.current_stream().cuda_stream

    def calls(self):
        L, p, st = self.L, (lambda t: t.data_ptr()), self.st
        gd, ad = ctypes.byref(self.gd), ctypes.byref(self.ad)
        return {
            "gather fwd": lambda: lib.check(L.gs_ocr_gather_forward(
                gd, p(self.logits), p(self.feats), p(self.ctx), p(self.stats), p(self.ws), self.need, st), "gf"),
            "gather bwd": lambda: lib.check(L.gs_ocr_gather_backward(
                gd, p(self.logits), p(self.feats), p(self.ctx), p(self.stats), p(self.dctx), p(self.dl),
                p(self.df), 0, p(self.ws), self.need, st), "gb"),
            "attend fwd": lambda: lib.check(L.gs_ocr_attend_forward(
                ad, p(self.q), p(self.k), p(self.v), p(self.out), p(self.lse), st), "af"),
            "attend bwd": lambda: lib.check(L.gs_ocr_attend_backward(
                ad, p(self.q), p(self.k), p(self.v), p(self.out), p(self.lse), p(self.dout), p(self.dq),
                p(self.dk), p(self.dv), p(self.ws), self.need, st), "ab"),
        }

    def copy_of(self, nbytes):
        """gs_copy2d moving ``nbytes`` in all (half read, half written) on rows of 512 floats"""
        rows = max(1, nbytes // 2 // (512 * F4))
        src, dst = torch.empty(rows, 512, device="cuda"), torch.empty(rows, 512, device="cuda")
        return lambda: lib.check(self.L.gs_copy2d(src.data_ptr(), 512, dst.data_ptr(), 512, rows, 512, 1.0, 0,
                                                  self.st), "copy")


def torch_ops(o):
    """the torch compositions on the same data: forward, and forward + backward minus forward"""
    lg = o.logits[..., :K].clone().requires_grad_(True)
    ft = o.feats.clone().requires_grad_(True)
    q, k, v = (t.clone().requires_grad_(True) for t in (o.q, o.k, o.v))

    def gather():
        return torch.bmm(torch.softmax(lg.transpose(1, 2), dim=2), ft)

    def attend():
        return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * CH ** -0.5, dim=2), v)

    def fb(fn, grad, leaves):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward(grad)
        return run
    return {"gather fwd": lambda: gather().detach(), "gather fwd+bwd": fb(gather, o.dctx, (lg, ft)),
            "attend fwd": lambda: attend().detach(), "attend fwd+bwd": fb(attend, o.dout, (q, k, v))}


def med(v):
    return sorted(v)[len(v) // 2]


def bench_ops(iters, rounds=3):
    o = Ops()
    calls, tc, nbytes = o.calls(), torch_ops(o), call_bytes()
    copies = {k: o.copy_of(n) for k, n in nbytes.items()}
    for fn in calls.values():      # the backward calls read what the forward calls wrote
        fn()
    t = {k: [] for k in calls}
    tcp = {k: [] for k in calls}
    tt = {k: [] for k in tc}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(1000 * _time(fn, iters))
            tcp[k].append(1000 * _time(copies[k], iters))
        for k, fn in tc.items():
            tt[k].append(1000 * _time(fn, iters))
    return ({k: med(v) for k, v in t.items()}, {k: med(v) for k, v in tcp.items()}, {k: med(v) for k, v in tt.items()},
            nbytes, o)


def loop_ops(n):
    o = Ops()
    calls = o.calls()
    for _ in range(n):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()


def kernel_table(path, o, iters):
    """per-kernel rows from a rocprofv3 kernel-statistics CSV (columns Name, Calls, AverageNs)"""
    rows = list(csv.DictReader(open(path)))
    lines = ["| call | kernel | us per launch | MB to move | gs_copy2d of those bytes, us | kernel / copy |",
             "|---|---|---|---|---|---|"]
    for call, key, mult, n in kernel_bytes():
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            lines.append("| %s | %s | not in the trace | %.2f | | |" % (call, key, n / 1e6))
            continue
        us = sum(float(r["AverageNs"]) * float(r["Calls"]) for r in hit) / sum(float(r["Calls"]) for r in hit) / 1e3
        if n < 1 << 20:
            lines.append("| %s | %s | %.1f | %.2f | (below 1 MB: launch-bound) | |" % (call, key, us, n / 1e6))
            continue
        per = n // mult       # (several launches under one name: the mean launch against the mean bytes)
        cp = 1000 * _time(o.copy_of(per), iters)
        lines.append("| %s | %s%s | %.1f | %.2f | %.1f | %.2f |" % (call, key, " (mean of %d)" % mult if mult > 1 else "",
                                                                  us, per / 1e6, cp, us / cp))
    return lines


def bench_heads(iters, rounds=3):
    """ms of forward + backward (input and parameter gradients) of each head alone on random stage-4 features
    of the R50 anchor's width; the OCR head also reads random stage-0 logits (their gradient included)"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_head
    torch.manual_seed(0)
    x = torch.randn(B, 2048, H, W, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    prev = (3.0 * torch.randn(B, K, H, W, device="cuda")).requires_grad_(True)
    feats = [None, None, None, x]
    cfgs = {k: Config.fromfile(os.path.join(ROOT, "configs", "supernet", f)) for k, f in CONFIGS.items()}
    aspp = build_head(dict(cfgs["DeepLabV3"].model["decode_head"], dropout_ratio=0.0)).cuda().train()
    ocr = build_head(dict(cfgs["OCRNet"].model["decode_head"][1], dropout_ratio=0.0)).cuda().train()

    def step(head, *extra):
        def run():
            for p in head.parameters():
                p.grad = None
            x.grad = prev.grad = None
            out = head(feats, *extra)
            out.backward(torch.ones_like(out))
        return run
    fns = {"DynamicASPPHead": step(aspp), "DynamicOCRHead": step(ocr, prev)}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_time(fn, iters))
    return {k: med(v) for k, v in t.items()}


def bench_steps(args):
    """images/s of the training step on the R50 anchor, the two configs interleaved"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-heads", action="store_true")
    ap.add_argument("--loop-ops", type=int, default=0, help="only run the four calls N times (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="kernel statistics CSV of a rocprofv3 run of --loop-ops")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "r22_ocr_head.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ocr.py measures on the GPU: no device found")
    if args.loop_ops:
        loop_ops(args.loop_ops)
        return
    t, tcp, tt, nbytes, o = bench_ops(args.op_iters)
    lines = ["# OCRNet's region operators, head and recipe on the MI355X (tools/bench_ocr.py)", "",
             "Shape: bs %d, %dx%d pixels, K = %d, C = %d, ch = %d, fp32." % (B, H, W, K, C, CH), "",
             "## The four C-ABI calls (an event pair per call; median of 3 interleaved rounds of %d calls, us)"
             % args.op_iters, "",
             "| call | launches | us per call | MB to move | gs_copy2d of those bytes, us | call / copy |",
             "|---|---|---|---|---|---|"]
    launches = {"gather fwd": 4, "gather bwd": 2, "attend fwd": 1, "attend bwd": 5}
    for k in t:
        lines.append("| %s | %d | %.1f | %.1f | %.1f | %.2f |" % (k, launches[k], t[k], nbytes[k] / 1e6, tcp[k],
                                                                   t[k] / tcp[k]))
    lines += ["", "The bytes are what the call's kernels must move, partials between two of its kernels included: "
              "inputs read once, outputs written once.  The copy reads half of them and writes half.", ""]
    lines += ["## Per kernel (rocprofv3 --kernel-trace --stats on `--loop-ops`, a run of its own)", ""]
    if args.kernel_stats:
        lines += kernel_table(args.kernel_stats, o, args.op_iters)
    else:
        lines += ["Not measured in this run (no --kernel-stats file given)."]
    lines += ["", "## Each operator next to its torch composition (softmax + bmm, autograd), same process, us", "",
              "| operator | HIP forward | torch forward | HIP forward + backward | torch forward + backward |",
              "|---|---|---|---|---|"]
    for op in ("gather", "attend"):
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f |" % (op, t[op + " fwd"], tt[op + " fwd"],
                                                            t[op + " fwd"] + t[op + " bwd"], tt[op + " fwd+bwd"]))
    lines.append("")
    del o
    torch.cuda.empty_cache()
    if not args.skip_heads:
        hd = bench_heads(args.iters)
        lines += ["## The heads alone, forward + backward on random stage-4 features of the R50 anchor (2048 "
                  "channels), bs 2 (median of 3 interleaved rounds of %d, ms)" % args.iters, "",
                  "| " + " | ".join(hd) + " |", "|" + "---|" * len(hd),
                  "| " + " | ".join("%.2f" % v for v in hd.values()) + " |", ""]
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
