#!/usr/bin/env python
"""Channel-wise distillation (gs_cwd_*) on the GPU, HIP events throughout:
  * the forward and the backward alone at N=2, C=19, 64x128 and at N=2, C=150, 128x128 (padded
    channels-last views, as the decode head hands them over), next to a device-to-device copy of one
    logit map (the bytes the forward reads per map, moved) and to the same loss composed from torch's
    softmax ops on the GPU (forward, and forward + backward);
  * the distilled training step of configs/supernet/pspnet_ar50to101v2_distiller_cwd.py (R50 student
    under the MAX teacher, 1024x512, bs 2) with and without the channel loss, interleaved;
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout
    and of this one, alternately, each run a process of its own (the default path is untouched, so
    the two should agree within the box's noise).
Writes profiles/r12_cwd.md (--md).

    python tools/bench_cwd.py [--op-iters 200] [--iters 8] [--warmup 3] [--ab-runs 3] [--parent DIR]
                              [--bench-rounds 3] [--md profiles/r12_cwd.md]"""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402
from gaia_seg_amd.models.losses.distill_loss import channel_distill_loss, cwd_desc  # noqa: E402

LAUNCHES = {"gs_cwd_forward": 3, "gs_cwd_backward": 1}   # csrc/cwd.hip: independent of the sizes
SHAPES = [(2, 19, 64, 128), (2, 150, 128, 128)]


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


def torch_cwd(s, t, T, weight):
    n, c = s.shape[:2]
    ls = torch.log_softmax(s.reshape(n * c, -1) / T, dim=1)
    lt = torch.log_softmax(t.reshape(n * c, -1) / T, dim=1)
    return weight * T * T / (n * c) * torch.sum(lt.exp() * (lt - ls))


def bench_ops(iters, rounds=3):
    L = lib.load()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    torch.manual_seed(0)
    for n, c, h, w in SHAPES:
        ld = (c + 3) // 4 * 4
        sbuf = torch.randn(n, h, w, ld, device=dev) * 2
        tbuf = torch.randn(n, h, w, ld, device=dev) * 2
        s, t = sbuf.permute(0, 3, 1, 2)[:, :c], tbuf.permute(0, 3, 1, 2)[:, :c]
        d = cwd_desc(s, t, 1.0)
        lse_s = torch.empty(n, c, device=dev)
        lse_t = torch.empty_like(lse_s)
        out = torch.empty(1, device=dev)
        ws = torch.empty(L.gs_cwd_workspace_bytes(ctypes.byref(d)) // 4 + 64, device=dev)
        buf = torch.empty(n, h, w, ld, device=dev)
        dst = torch.empty_like(sbuf)
        sg = s.detach().requires_grad_(True)

        def fwd():
            lib.check(L.gs_cwd_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                       lse_t.data_ptr(), 1e-2, out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                       st), "gs_cwd_forward")

        def bwd():
            lib.check(L.gs_cwd_backward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                                        lse_t.data_ptr(), 1e-2, buf.data_ptr(), ld, st), "gs_cwd_backward")

        def copy():
            dst.copy_(sbuf)

        def torch_fwd():
            with torch.no_grad():
                torch_cwd(s, t, 1.0, 5.0)

        def torch_fwd_bwd():
            sg.grad = None
            torch_cwd(sg, t, 1.0, 5.0).backward()

        def hip_fwd_bwd():
            sg.grad = None
            channel_distill_loss(sg, t, T=1.0, weight=5.0).backward()
        fns = dict(fwd=fwd, bwd=bwd, copy=copy, torch_fwd=torch_fwd, torch_fwd_bwd=torch_fwd_bwd,
                   hip_fwd_bwd=hip_fwd_bwd)
        best = {k: [] for k in fns}
        for _ in range(rounds):          # interleaved rounds in one process; the median is reported
            for k, fn in fns.items():
                best[k].append(1000 * _time(fn, iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in best.items()}
        # the loss agrees with the composition before its time is compared with it
        ref = float(torch_cwd(s.double(), t.double(), 1.0, 5.0))
        got = float(channel_distill_loss(s, t, T=1.0, weight=5.0))
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        rows.append(dict(shape=(n, c, h, w), ld=ld, map_mb=n * h * w * ld * 4 / 1e6,
                         parts=L.gs_cwd_debug_partials(ctypes.byref(d)), **med))
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
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.synthetic import make_batch
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller_cwd.py"))
    batch = make_batch(2, 512, 1024, seed=0, device="cuda")
    tmp = tempfile.mkdtemp()
    try:
        return _bench_steps(args, cfg, batch, os.path.join(tmp, "teacher.pth"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _bench_steps(args, cfg, batch, ck):
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    tcfg = dict(cfg.model["teacher_segmentor"], test_cfg=dict(mode="whole"))
    save_checkpoint(build_segmentor(tcfg), ck)       # random weights: the timing does not depend on them

    def build(**over):
        m = dict(cfg.model, teacher_ckpt=ck)
        m.update(over)
        torch.manual_seed(0)
        return build_segmentor(m, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg")).cuda().train()
    meta = anchor(cfg, "R50")
    r_on, r_off = _runner(build(), meta), _runner(build(has_channel_loss=False), meta)
    out = r_on.train_iter(batch)
    assert "channel_loss_seg" in out["log_vars"]
    assert "channel_loss_seg" not in r_off.train_iter(batch)["log_vars"]
    _time(lambda: r_on.train_iter(batch), args.warmup, 0)
    _time(lambda: r_off.train_iter(batch), args.warmup, 0)
    ab = {"on": [], "off": []}
    for _ in range(args.ab_runs):      # interleaved: with, without, with, ...
        ab["on"].append(_time(lambda: r_on.train_iter(batch), args.iters, 1))
        ab["off"].append(_time(lambda: r_off.train_iter(batch), args.iters, 1))
    return ab


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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=200)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "r12_cwd.md"))
    args = ap.parse_args()
    # before this process touches the GPU: every bench.py run has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    lib.load()
    lines = ["# Channel-wise distillation on the MI355X (tools/bench_cwd.py)", "",
             "## The operator alone (padded channels-last views, T = 1; median of 3 interleaved rounds of "
             "%d calls, us per call)" % args.op_iters, "",
             "| N, C, H x W | one map MB | ranges per map | forward (%d launches) | backward (%d launch) | "
             "copy of one map | forward / copy | torch forward | torch forward + backward | "
             "autograd wrapper forward + backward |" % (LAUNCHES["gs_cwd_forward"], LAUNCHES["gs_cwd_backward"]),
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in bench_ops(args.op_iters):
        lines.append("| %d, %d, %dx%d | %.2f | %d | %.1f | %.1f | %.1f | %.2f | %.1f | %.1f | %.1f |"
                     % (r["shape"] + (r["map_mb"], r["parts"], r["fwd"], r["bwd"], r["copy"],
                                      r["fwd"] / r["copy"], r["torch_fwd"], r["torch_fwd_bwd"],
                                      r["hip_fwd_bwd"])))
    lines += ["", "The forward reads two maps once and writes nothing of their size; the copy reads one map and "
              "writes one (the same bytes moved).  The autograd wrapper adds the allocation of the gradient "
              "buffer and one elementwise launch (the upstream scalar, applied on the device).", ""]
    if not args.skip_steps:
        ab = bench_steps(args)
        on, off = ab["on"], ab["off"]
        lines += ["## Distilled training step, PSP supernet, R50 student under the MAX teacher, 1024x512, bs 2 "
                  "(interleaved, %d runs of %d iterations, ms per step)" % (args.ab_runs, args.iters), "",
                  "| logit loss + channel loss | logit loss alone | difference of the means |", "|---|---|---|",
                  "| %s (mean %.2f) | %s (mean %.2f) | %+.2f |"
                  % (" ".join("%.2f" % v for v in on), sum(on) / len(on), " ".join("%.2f" % v for v in off),
                     sum(off) / len(off), sum(on) / len(on) - sum(off) / len(off))]
    lines += ["", "## `bench.py --gpus 1 --steps 32 --warmup 8`, parent commit against this commit "
              "(alternating, one process per run, images/s)", ""]
    if ab_py:
        p, t = ab_py["parent"], ab_py["this"]
        lines += ["| parent | this commit |", "|---|---|",
                  "| %s (mean %.2f) | %s (mean %.2f) |" % (" ".join("%.2f" % v for v in p), sum(p) / len(p),
                                                         " ".join("%.2f" % v for v in t), sum(t) / len(t))]
    else:
        lines += ["Not measured in this run (no --parent checkout given)."]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
