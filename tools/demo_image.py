#!/usr/bin/env python
"""Segment one image and draw the result over it -- the reference's demo flow
(gaiaseg/apis/inference.py: init_segmentor, inference_segmentor, show_result).

    python tools/demo_image.py IMG CONFIG CHECKPOINT [--arch NAME|JSON] [--out result.png] [--opacity 0.5]

``--arch``: which subnet of a supernet checkpoint to run: the name of an anchor of the config's
samplers or a JSON meta; a config with ``model_sampler`` or an extracted subnet needs none.  The
config's ``data.test.pipeline`` decides the views (multi-scale / flip included)."""
import argparse
import json
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

from gaia_seg_amd.apis.inference import inference_segmentor, init_segmentor  # noqa: E402
from gaia_seg_amd.core.config import Config, DictAction  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Segment an image and save the overlay")
    ap.add_argument("img")
    ap.add_argument("config")
    ap.add_argument("checkpoint")
    ap.add_argument("--arch", default=None, help="anchor name or JSON meta of the subnet to run")
    ap.add_argument("--out", default="result.png", help="where the blended image goes")
    ap.add_argument("--opacity", type=float, default=0.5, help="opacity of the label colours, (0, 1]")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--cfg-options", nargs="+", default=None)
    args = ap.parse_args(argv)
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(DictAction.parse(args.cfg_options))
    arch = args.arch
    if arch is not None and arch.lstrip().startswith("{"):
        arch = json.loads(arch)
    model = init_segmentor(cfg, args.checkpoint, device=args.device, arch=arch)
    result = inference_segmentor(model, args.img)
    model.show_result(args.img, result, opacity=args.opacity, out_file=args.out)
    print("wrote %s (%d x %d, %d classes present)" % (args.out, result[0].shape[1], result[0].shape[0],
                                                     len(set(result[0].ravel().tolist()))))


if __name__ == "__main__":
    main()
