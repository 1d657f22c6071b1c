#!/usr/bin/env python
"""Eval-forward throughput of the FCN supernet (configs/supernet/fcn_ar50to101v2.py) in fp32 and
with fp16 conv operands (gs_set_forward_precision(1), core.fp16_utils.wrap_fp16_model):

    python tools/bench_eval.py [--anchors MIN,R50,MAX] [--iters 10] [--shapes] [--md out.md]

Per anchor: images/s of simple_test_device on one whole 1024x2048 image (random weights, eval-mode
BatchNorm), both precisions, and the share of the conv FLOPs (2*M*N*K) that ran on the f16 loop in
the fp16 pass.  --shapes adds the forward of every R50 / MAX / MIN bottleneck conv shape at
1024x2048 (bs 1), kernel alone (HIP events, 30 launches), fp32 against fp16, with the K loop taken.
bench.py (the training headline) is not involved."""
import argparse
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

KLOOP = {0: "generic", 1: "fp32", 2: "fp32x2", 3: "bf16x3", 4: "stream", 5: "f16"}
RES = [(256, 512), (128, 256), (64, 128), (32, 64)]
WIDTHS = {"R50": [64, 128, 256, 512], "MAX": [80, 160, 320, 640], "MIN": [48, 96, 192, 384]}


def anchor_arch(cfg, name):
    from gaia_seg_amd.core.dynamic import fold_dict
    for m in cfg.train_sampler["model_samplers"][0]["anchors"]:   # the anchor list of the sampler
        if m.get("name") == name:
            return fold_dict(dict(m))["arch"]
    raise KeyError(name)


def conv_flops(L):
    buf = (ctypes.c_double * (3 * lib.KLOOP_COUNT))()
    L.gs_debug_conv_launch_flops(buf, 0)
    n = ctypes.c_int64()
    f16 = ctypes.c_double()
    L.gs_debug_f16_launches(ctypes.byref(n), ctypes.byref(f16), 0)
    return sum(buf[lib.OP_FORWARD * lib.KLOOP_COUNT + k] for k in range(lib.KLOOP_COUNT)), f16.value


def bench_anchors(args, L):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    torch.manual_seed(0)
    model = model.cuda().eval()
    img = torch.randn(1, 3, 1024, 2048, device="cuda")
    metas = [dict(ori_shape=(1024, 2048, 3), img_shape=(1024, 2048, 3), pad_shape=(1024, 2048, 3),
                  flip=False)]
    rows = []
    for name in args.anchors.split(","):
        model.manipulate_arch(anchor_arch(cfg, name))
        res = {}
        for prec in ("fp32", "fp16"):
            model.fp16_enabled = False
            if prec == "fp16":
                wrap_fp16_model(model)
            with torch.no_grad():
                for _ in range(3):
                    model.simple_test_device(img, metas)
                torch.cuda.synchronize()
                L.gs_debug_conv_launch_flops(None, 1)
                L.gs_debug_f16_launches(None, None, 1)
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    model.simple_test_device(img, metas)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.iters
            fl32, fl16 = conv_flops(L)
            res[prec] = (1.0 / dt, fl16 / max(fl32 + fl16, 1.0))
        model.fp16_enabled = False
        rows.append((name, res["fp32"][0], res["fp16"][0], res["fp16"][0] / res["fp32"][0], res["fp16"][1]))
        print("%-5s fp32 %6.2f img/s  fp16 %6.2f img/s  x%.3f  f16 share of conv FLOPs %.3f" % rows[-1],
              flush=True)
    return rows


def bench_shapes(args, L):
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for wname in args.anchors.split(","):
        ws = WIDTHS[wname]
        for s, (h, w) in enumerate(RES):
            wd = ws[s]
            cases = [("%s s%d conv2 3x3 %d" % (wname, s + 1, wd), h, w, wd, wd, 3, 1, True),
                     ("%s s%d conv3 1x1 %d->%d aff" % (wname, s + 1, wd, 4 * wd), h, w, wd, 4 * wd, 1, 1, True),
                     ("%s s%d conv1 1x1 %d->%d" % (wname, s + 1, 4 * wd, wd), h, w, 4 * wd, wd, 1, 1, False)]
            if s > 0:
                ph, pw = RES[s - 1]
                cases.append(("%s s%d.0 conv2 3x3/2 %d" % (wname, s + 1, wd), ph, pw, wd, wd, 3, 2, True))
            for name, hh, ww, ci, co, k, stride, aff in cases:
                d = lib.conv_desc(1, hh, ww, ci, co, k, stride, role=1 if k == 3 else 0)
                x = torch.randn(1, hh, ww, ci, device=dev)
                y = torch.empty(1, d.Ho, d.Wo, co, device=dev)
                wt = torch.randn(k, k, ci, co, device=dev) * 0.05
                coeffs = torch.stack([torch.ones(ci), torch.zeros(ci), torch.zeros(ci), torch.ones(ci)]).to(dev)
                if aff and L.gs_conv2d_in_affine_supported(ctypes.byref(d)):
                    d.in_affine = coeffs.data_ptr()
                need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
                wsb = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
                fl = 2.0 * d.Ho * d.Wo * ci * co * k * k
                out = [name]
                for mode in (0, 1):
                    L.gs_set_forward_precision(mode)
                    try:
                        def run():
                            return L.gs_conv2d_forward(ctypes.byref(d), x.data_ptr(), wt.data_ptr(), None, None,
                                                       y.data_ptr(), wsb.data_ptr(), wsb.numel(), st)
                        for _ in range(5):
                            lib.check(run(), "fwd")
                        rec = lib.DebugLaunch()
                        L.gs_debug_last_conv_launch(ctypes.byref(rec))
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(30):
                            run()
                        e1.record()
                        torch.cuda.synchronize()
                    finally:
                        L.gs_set_forward_precision(0)
                    us = e0.elapsed_time(e1) * 1e3 / 30
                    out += [us, fl / us / 1e6, "%s 64x%d s%d" % (KLOOP.get(rec.kloop, "?"), rec.bn, rec.splits)]
                out.append(out[1] / out[4])
                rows.append(tuple(out))
                print("%-30s fp32 %7.1f us %6.1f TF %-16s fp16 %7.1f us %6.1f TF %-16s x%.2f" % rows[-1],
                      flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", default="MIN,R50,MAX")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    L = lib.load()
    arows = bench_anchors(args, L)
    srows = bench_shapes(args, L) if args.shapes else []
    if args.md:
        with open(args.md, "w") as f:
            f.write("| anchor | fp32 img/s | fp16 img/s | speed-up | f16 share of conv FLOPs |\n|---|---|---|---|---|\n")
            for r in arows:
                f.write("| %s | %.2f | %.2f | %.3f | %.3f |\n" % r)
            if srows:
                f.write("\n| shape (1024x2048, bs 1) | fp32 us | fp32 TF | fp32 kernel | fp16 us | fp16 TF | "
                        "fp16 kernel | speed-up |\n|---|---|---|---|---|---|---|---|\n")
                for r in srows:
                    f.write("| %s | %.1f | %.1f | %s | %.1f | %.1f | %s | %.2f |\n" % r)


if __name__ == "__main__":
    main()
