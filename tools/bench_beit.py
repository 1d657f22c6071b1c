#!/usr/bin/env python
"""The BEiT teacher on the GPU, HIP events throughout:
  * gs_attention_relpos_forward against gs_attention_forward at the same shapes -- of this build and, with
    --parent-lib, of the parent commit's library loaded beside it (one process, interleaved rounds);
  * gs_deconv2x2_forward at the two fpn1 shapes of BEiT-B/16 on a 512x1024 crop, next to torch-ROCm's
    F.conv_transpose2d (channels_last) on the same device and data;
  * the teacher's forward (BEiT-B/16 + UPerHead of configs/supernet/upernet_elastic_vit_distiller_beit.py,
    512x1024, bs 2, under no_grad);
  * the training step of that config against the plain configs/supernet/upernet_elastic_vit_adamw.py,
    each in a process of its own, alternating (the teacher is loaded from a checkpoint of random weights
    written for the run);
  * with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` of that checkout and
    of this one, alternately, one process per run.
Writes its tables to --md (default work_dirs/bench_beit.md); profiles/r18_beit_teacher.md holds the tables
of one run with the reading of them.

    python tools/bench_beit.py [--op-iters 30] [--steps 6] [--passes 2] [--parent-lib SO] [--parent DIR]
                               [--bench-rounds 3] [--skip-steps] [--md FILE]"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaia_seg_amd.hip import lib  # noqa: E402

CFG_DISTILL = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit_distiller_beit.py")
CFG_PLAIN = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit_adamw.py")
N, H, W = 2, 512, 1024
# (name, B, Wh, Ww, heads)
ATTENTION_SHAPES = [("BEiT-B/16 224^2", 8, 14, 14, 12), ("BEiT-B/16 512x1024", 2, 32, 64, 12),
                    ("BEiT-L/16 640^2", 1, 40, 40, 16)]
# (name, N, H, W, Cin, Cout)
DECONV_SHAPES = [("fpn1.0 / fpn2.0", 2, 32, 64, 768, 768), ("fpn1.3", 2, 64, 128, 768, 768)]


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


def _median_rounds(fns, iters, rounds=5):
    """{name: (median, min, max) us per call} over ``rounds`` interleaved rounds"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(1000 * _time(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def bench_attention(iters, parent_lib):
    L = lib.load()
    P = None
    if parent_lib:
        P = ctypes.CDLL(parent_lib)
        P.gs_attention_forward.restype, P.gs_attention_forward.argtypes = lib.PROTOTYPES["gs_attention_forward"]
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, b, wh, ww, heads in ATTENTION_SHAPES:
        n, c = wh * ww + 1, 64 * heads
        qkv = torch.randn(b, n, 3 * c, device="cuda")
        q, k, v = (qkv.data_ptr() + 4 * i * c for i in range(3))
        o = torch.empty(b, n, c, device="cuda")
        lse = torch.empty(b * heads * n, device="cuda")
        table = torch.randn((2 * wh - 1) * (2 * ww - 1) + 3, heads, device="cuda")
        d = lib.attention_desc(b, n, heads, ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c)
        db = ctypes.byref(d)
        fns = dict(
            plain=lambda: lib.check(L.gs_attention_forward(db, q, k, v, o.data_ptr(), lse.data_ptr(), st), "plain"),
            relpos=lambda: lib.check(L.gs_attention_relpos_forward(db, q, k, v, table.data_ptr(), heads, wh, ww,
                                                                   o.data_ptr(), lse.data_ptr(), st), "relpos"))
        if P is not None:
            fns["parent"] = lambda: lib.check(P.gs_attention_forward(db, q, k, v, o.data_ptr(), lse.data_ptr(), st),
                                              "parent")
        med = _median_rounds(fns, iters)
        flops = 4.0 * b * heads * n * n * 64
        rows.append(dict(name=name, shape="%d x %d x %d heads" % (b, n, heads), med=med, flops=flops))
        print(name, {k: "%.1f us" % m[0] for k, m in med.items()}, flush=True)
    return rows


def bench_deconv(iters):
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, n, h, w, cin, cout in DECONV_SHAPES:
        x = torch.randn(n, h, w, cin, device="cuda")
        wt = torch.randn(cin, cout, 2, 2, device="cuda") / cin ** 0.5
        w4 = wt.permute(0, 2, 3, 1).contiguous()
        bias = torch.randn(cout, device="cuda")
        y = torch.empty(n, 2 * h, 2 * w, cout, device="cuda")
        need = L.gs_deconv2x2_workspace_bytes(n, h, w, cin, cout)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        xt = x.permute(0, 3, 1, 2)                         # NCHW view of NHWC storage = channels_last
        fns = dict(
            ours=lambda: lib.check(L.gs_deconv2x2_forward(x.data_ptr(), n, h, w, cin, cin, w4.data_ptr(), cout,
                                                          bias.data_ptr(), y.data_ptr(), cout, ws.data_ptr(), need,
                                                          st), "deconv"),
            torch=lambda: F.conv_transpose2d(xt, wt, bias, stride=2))
        med = _median_rounds(fns, iters)
        rows.append(dict(name=name, shape="%d x %d x %d, %d -> %d" % (n, h, w, cin, cout), med=med,
                         flops=2.0 * n * h * w * cin * 4 * cout))
        print(name, {k: "%.1f us" % m[0] for k, m in med.items()}, flush=True)
    return rows


def _cfg(path):
    from gaia_seg_amd.core.config import Config
    return Config.fromfile(path)


def write_teacher(path):
    """the config's teacher with its constructor's (random) weights and random tables, as a checkpoint"""
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    cfg = _cfg(CFG_DISTILL)
    torch.manual_seed(1)
    t = build_segmentor(cfg.model.teacher_segmentor, test_cfg=cfg.get("test_cfg"))
    with torch.no_grad():
        for blk in t.backbone.blocks:
            blk.attn.relative_position_bias_table.normal_(0, 0.5)
    save_checkpoint(t, path)
    return t


def bench_teacher(teacher, iters):
    teacher = teacher.cuda().eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    img = torch.randn(N, 3, H, W, device="cuda")

    def backbone():
        with torch.no_grad():
            teacher.backbone(img)

    def whole():
        with torch.no_grad():
            teacher._decode_head_forward_test(teacher.extract_feat(img), None)
    return _median_rounds(dict(backbone=backbone, whole=whole), iters, rounds=3)


def steps_child(kind, steps, ckpt):
    """one process, one model: images/s of the training step on the config's largest subnet"""
    from bench_adamw import make_runner
    cfg = _cfg(CFG_DISTILL if kind == "distill" else CFG_PLAIN)
    if kind == "distill":
        cfg.model["teacher_ckpt"] = ckpt
    runner = make_runner(cfg, cfg.optimizer)
    g = torch.Generator().manual_seed(0)
    batch = dict(img=torch.randn(N, 3, H, W, generator=g).cuda(),
                 img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False)
                            for _ in range(N)],
                 gt_semantic_seg=torch.randint(0, 19, (N, 1, H, W), generator=g).cuda())
    for _ in range(3):
        runner.train_iter(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner.train_iter(batch)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(N * steps / (time.perf_counter() - t0)), flush=True)


def bench_steps(args, ckpt):
    res = {"plain": [], "distill": []}
    for _ in range(args.passes):
        for kind in res:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(args.steps),
                   "--ckpt", ckpt]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                raise SystemExit("child %s failed (exit %d):\n%s" % (kind, r.returncode, r.stderr[-2000:]))
            res[kind].append(json.loads(line[-1][7:]))
            print("step %s: %.2f images/s" % (kind, res[kind][-1]), flush=True)
    return res


def bench_py_ab(parent, rounds, steps=32, warmup=8):
    """images/s of `bench.py` in ``parent`` and in this checkout, alternately, one process per run; the
    round's first run changes sides every round."""
    out = {"parent": [], "this": []}
    pair = [("parent", parent), ("this", ROOT)]
    for rnd in range(rounds):
        for name, root in (pair if rnd % 2 == 0 else pair[::-1]):
            res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
                                  "--warmup", str(warmup)], cwd=root, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                raise RuntimeError("bench.py failed in %s:\n%s" % (root, res.stderr[-2000:]))
            out[name].append(json.loads(res.stdout.strip().splitlines()[-1])["value"])
            print("bench.py %s: %.2f images/s" % (name, out[name][-1]), flush=True)
    return out


def _runs(v, fmt="%.2f"):
    return "%s (median %s)" % (" ".join(fmt % x for x in v), fmt % statistics.median(v))


def _us(m):
    return "%.1f (%.1f..%.1f)" % m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op-iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-teacher", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libgaiaseg_hip.so of the parent commit")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (bench.py A/B)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(ROOT, "work_dirs", "bench_beit.md"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--ckpt", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return steps_child(args.child, args.steps, args.ckpt)
    # before this process touches the GPU: every bench.py run and every step child has the device to itself
    ab_py = bench_py_ab(os.path.abspath(args.parent), args.bench_rounds) if args.parent else None
    tmp = tempfile.mkdtemp(prefix="bench_beit_")
    ckpt = os.path.join(tmp, "beit_b16_upernet_random.pth")
    teacher = None
    if not (args.skip_steps and args.skip_teacher):
        teacher = write_teacher(ckpt)
    steps = None if args.skip_steps else bench_steps(args, ckpt)
    lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_beit.py measures on the GPU: no device found")
    lines = ["## Attention forward with and without the relative-position bias (fp32, head dimension 64, Q / K / V "
             "as slices of one buffer; median (min..max) of 5 interleaved rounds of %d calls, us per call)"
             % args.op_iters, "",
             "| shape | B x N x heads | bias-free, parent commit | bias-free, this commit | biased | biased / "
             "parent's bias-free | biased TFLOP/s |", "|---|---|---|---|---|---|---|"]
    for r in bench_attention(args.op_iters, args.parent_lib):
        m = r["med"]
        base = m.get("parent", m["plain"])
        lines.append("| %s | %s | %s | %s | %s | %.3f%s | %.1f |" % (
            r["name"], r["shape"], _us(m["parent"]) if "parent" in m else "not measured", _us(m["plain"]),
            _us(m["relpos"]), m["relpos"][0] / base[0], "" if "parent" in m else " (of this commit's)",
            r["flops"] / m["relpos"][0] / 1e6))
    lines += ["", "## ConvTranspose2d(2, 2) forward (fp32 NHWC, bs 2 at 512x1024; us per call, as above)", "",
              "| layer | N x H x W, Cin -> Cout | ours (GEMM + depth-to-space) | torch conv_transpose2d | ours / torch "
              "| ours TFLOP/s |", "|---|---|---|---|---|---|"]
    for r in bench_deconv(args.op_iters):
        m = r["med"]
        lines.append("| %s | %s | %s | %s | %.2f | %.1f |" % (r["name"], r["shape"], _us(m["ours"]), _us(m["torch"]),
                                                              m["ours"][0] / m["torch"][0],
                                                              r["flops"] / m["ours"][0] / 1e6))
    lines += ["", "## The teacher's forward: BEiT-B/16 + UPerHead, 512x1024, bs 2, no_grad (ms per call)", ""]
    if teacher is not None and not args.skip_teacher:
        t = bench_teacher(teacher, 3)
        lines += ["| backbone | backbone + decode head |", "|---|---|",
                  "| %.1f | %.1f |" % (t["backbone"][0] / 1e3, t["whole"][0] / 1e3)]
    else:
        lines += ["Not measured in this run."]
    lines += ["", "## Training step, largest subnet, 512x1024, bs 2: upernet_elastic_vit_adamw.py against "
              "upernet_elastic_vit_distiller_beit.py (one process per run, alternating, images/s)", ""]
    if steps:
        a, b = statistics.median(steps["plain"]), statistics.median(steps["distill"])
        lines += ["| plain | distilled | distilled / plain | teacher's share of a distilled step |", "|---|---|---|---|",
                  "| %s | %s | %.3f | %.1f ms of %.1f ms |" % (_runs(steps["plain"]), _runs(steps["distill"]), b / a,
                                                              1e3 * N * (1 / b - 1 / a), 1e3 * N / b)]
    else:
        lines += ["Not measured in this run."]
    lines += ["", "## `bench.py --gpus 1 --steps 32 --warmup 8`, parent commit against this commit "
              "(alternating, one process per run, images/s)", ""]
    if ab_py:
        lines += ["| parent | this commit |", "|---|---|",
                  "| %s | %s |" % (_runs(ab_py["parent"]), _runs(ab_py["this"]))]
    else:
        lines += ["Not measured in this run (no --parent checkout given)."]
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
