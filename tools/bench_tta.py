#!/usr/bin/env python
"""Multi-scale + flip test-time augmentation, measured (profiles/r10_tta.md):

    python tools/bench_tta.py [--passes 5] [--images 3] [--anchor R50] [--no-eval] [--md out.md]

1. The view kernel: a 1024x2048 uint8 source and the 12-view ladder of
   configs/supernet/fcn_ar50to101v2_test_supernet_tta.py.  ``gs_tta_views`` (one launch) against the
   only way to make the same pixels without it: one ``gs_seg_augment`` launch per view (its
   horizontal flip for the mirrored views; it also reads a label map and writes an int64 label plane).
   Every launch is timed by an event pair around its own dispatch; the per-view side is the sum of
   its twelve launches.  The two sides alternate inside each pass; medians of ``--passes`` passes,
   with the spread (max - min) of the passes beside them.
2. Evaluation cost: images/s of the FCN supernet's ``--anchor`` (random weights, eval mode) on one
   1024x2048 image at 1 view (simple_test_device) and at the 12 views (tta_batch + aug_test_device),
   beside the FLOP ratio 2 * sum(r^2).  Recorded, not gated.
bench.py (the training headline) is not involved."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaia_seg_amd.hip import lib  # noqa: E402

H, W = 1024, 2048
RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


def ladder():
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.datasets import tta_pipeline_kwargs, tta_views
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_test_supernet_tta.py"))
    kw = tta_pipeline_kwargs(cfg.data.val.pipeline)
    return kw, tta_views(kw, H, W)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def bench_views(args, L):
    from gaia_seg_amd.datasets import GpuTrainPipeline
    from gaia_seg_amd.datasets.gpu_pipeline import rescale_size
    kw, views = ladder()
    pipe = GpuTrainPipeline(mean=kw["mean"], std=kw["std"], to_rgb=kw["to_rgb"], src_is_rgb=True,
                            photometric=False, flip_ratio=0.0)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    label = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    sizes = [rescale_size(H, W, v["scale"]) for v in views]
    outs = [torch.empty((3, rh, rw), dtype=torch.float32, device="cuda") for rh, rw in sizes]
    labs = [torch.empty((rh, rw), dtype=torch.int64, device="cuda") for rh, rw in sizes]
    d = lib.TtaDesc()
    d.src_h, d.src_w, d.src_is_rgb, d.n_views, d.to_rgb = H, W, 1, len(views), int(kw["to_rgb"])
    for k in range(3):
        d.mean[k], d.std[k] = kw["mean"][k], kw["std"][k]
    descs = []
    for k, (v, (rh, rw)) in enumerate(zip(views, sizes)):
        d.views[k].res_h, d.views[k].res_w = rh, rw
        d.views[k].flip = lib.FLIP_CODES[v["flip_direction"] if v["flip"] else None]
        d.views[k].out = outs[k].data_ptr()
        a = pipe.descriptor(H, W, dict(res_h=rh, res_w=rw, crop_y=0, crop_x=0, crop_h=rh, crop_w=rw,
                                       flip=v["flip"]), True)
        a.out_h, a.out_w = rh, rw
        descs.append(a)

    def one_launch():
        lib.check(L.gs_tta_views(d, img.data_ptr(), st), "gs_tta_views")

    def per_view(k):
        lib.check(L.gs_seg_augment(ctypes.byref(descs[k]), img.data_ptr(), label.data_ptr(),
                                   outs[k].data_ptr(), labs[k].data_ptr(), st), "gs_seg_augment")

    for _ in range(2):                       # warm-up; the second round's outputs are compared below
        for k in range(len(views)):
            per_view(k)
    want = [o.clone() for o in outs]
    one_launch()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(outs, want))
    new_us, old_us, old_span_us = [], [], []
    for p in range(args.passes):
        for side in ((0, 1) if p % 2 == 0 else (1, 0)):
            torch.cuda.synchronize()
            if side == 0:
                e = timed(one_launch)
                torch.cuda.synchronize()
                new_us.append(e[0].elapsed_time(e[1]) * 1e3)
            else:
                ev = [timed(lambda k=k: per_view(k)) for k in range(len(views))]
                torch.cuda.synchronize()
                old_us.append(sum(a.elapsed_time(b) for a, b in ev) * 1e3)
                old_span_us.append(ev[0][0].elapsed_time(ev[-1][1]) * 1e3)
    px = sum(rh * rw for rh, rw in sizes)

    def stat(xs):
        return statistics.median(xs), max(xs) - min(xs)
    res = dict(same=same, pixels=px, new=stat(new_us), old=stat(old_us), old_span=stat(old_span_us))
    print("views: %d, %.1f M output pixels; outputs bit-identical to the per-view launches: %s"
          % (len(views), px / 1e6, same))
    for name, key, bpp in (("gs_tta_views, 1 launch", "new", 12), ("gs_seg_augment x12, sum of launches", "old", 20),
                           ("gs_seg_augment x12, first start to last end", "old_span", 20)):
        med, spread = res[key]
        print("%-46s median %8.1f us  spread %6.1f us  (%.2f TB/s written)"
              % (name, med, spread, px * bpp / med / 1e6), flush=True)
    return res


def bench_eval(args):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.datasets import GpuTrainPipeline
    from gaia_seg_amd.models import build_segmentor
    kw, views = ladder()
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    torch.manual_seed(0)
    model = model.cuda().eval()
    arch = [m for m in cfg.val_sampler["anchors"] if m.get("name") == args.anchor]
    model.manipulate_arch(fold_dict(dict(arch[0]))["arch"])
    pipe = GpuTrainPipeline(mean=kw["mean"], std=kw["std"], to_rgb=kw["to_rgb"], src_is_rgb=True,
                            photometric=False, flip_ratio=0.0)
    g = torch.Generator().manual_seed(1)
    sample = (torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda(), None)

    def single():
        b = pipe.test_batch([sample], (W, H))
        return model.simple_test_device(b["img"], b["img_metas"])

    def tta():
        b = pipe.tta_batch([sample], views)
        return model.aug_test_device(b["img"], b["img_metas"])
    out = {}
    with torch.no_grad():
        for name, fn in (("1 view", single), ("%d views" % len(views), tta)):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.images):
                fn()
            torch.cuda.synchronize()
            out[name] = args.images / (time.perf_counter() - t0)
            print("%s %-9s %7.3f images/s" % (args.anchor, name, out[name]), flush=True)
    a, b = list(out.values())
    flop_ratio = len(kw["flips"]) * sum(r * r for r in RATIOS)
    print("measured cost ratio %.2f beside the FLOP ratio %.2f" % (a / b, flop_ratio))
    return dict(single=a, tta=b, ratio=a / b, flop_ratio=flop_ratio, views=len(views))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--anchor", default="R50")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    L = lib.load()
    v = bench_views(args, L)
    e = None if args.no_eval else bench_eval(args)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| 12 views of a 1024x2048 image (%.1f M output pixels) | median us | spread of %d passes us |\n"
                    "|---|---|---|\n" % (v["pixels"] / 1e6, args.passes))
            f.write("| gs_tta_views, one launch | %.1f | %.1f |\n" % v["new"])
            f.write("| gs_seg_augment, one launch per view, sum of the launches | %.1f | %.1f |\n" % v["old"])
            f.write("| gs_seg_augment, first start to last end | %.1f | %.1f |\n" % v["old_span"])
            f.write("\noutputs bit-identical: %s\n" % v["same"])
            if e:
                f.write("\n| %s, one 1024x2048 image | images/s |\n|---|---|\n| 1 view | %.3f |\n| %d views | %.3f |\n"
                        "\nmeasured ratio %.2f, FLOP ratio %.2f\n"
                        % (args.anchor, e["single"], e["views"], e["tta"], e["ratio"], e["flop_ratio"]))


if __name__ == "__main__":
    main()
