"""Generates tests/golden/convformer_relu_margin.json: BatchNorm bias values that keep every ReLU input of
the tiny ElasticConvformer of tests/test_convformer_gpu.py away from zero.  Run on a CPU:

    python tests/golden/make_convformer_relu_margin.py

Why: the gradient-parity test compares an fp32 GPU pass with a float64 CPU pass, which only makes sense when
both take the same branch of every ReLU, so it asserts that no ReLU input of the float64 pass lies within
1e-4 rms of zero.  The four passes of the test (subnets 'max' and 'sub', norm_eval on and off) see about a
million ReLU inputs; with a density of roughly 0.4 / rms at zero about 80 of them violate that margin for ANY
seed, so no seed satisfies the condition.  Instead, the inputs are made to satisfy it: the ReLUs are visited in
forward order, and where a channel of one has an input inside the margin in any of the four passes, the bias of
the BatchNorm in front of it (which shifts exactly that channel, in every pass, and nothing upstream) is moved
by the smallest multiple of 2.5e-4 rms that clears all four.  Only the float64 model of tests/util_convformer.py
is consulted.  The file holds the resulting fp32 bias values, as exact decimal strings of their doubles."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import util_convformer as U   # noqa: E402
from util_models import make_batch   # noqa: E402

TARGET = 1.2e-4    # of the rms; the test asserts 1e-4
STEP = 2.5e-4
PASSES = [(name, norm_eval) for name in ("max", "sub") for norm_eval in (True, False)]


def relu_inputs(model, img):
    """{bias name: [(tensor, rms)] over the passes that run that ReLU}, and the names in forward order"""
    sd = {k: v.detach().clone().double() for k, v in model.state_dict().items()}
    by_name, order = {}, []
    for name, norm_eval in PASSES:
        pre = []
        U.convformer_ref(sd, img, U.SUBNETS[name], norm_eval, relu_inputs=pre)
        for key, v in pre:
            if key not in by_name:
                by_name[key] = []
                order.append(key)
            by_name[key].append((v, float(v.pow(2).mean().sqrt())))
    return by_name, order


def main():
    from gaia_seg_amd.models import build_backbone
    model = build_backbone(U.tiny_backbone_cfg())
    U.randomize_convformer(model, U.SEED, margin=False)
    params = dict(model.named_parameters())
    img = make_batch(2, U.H, U.W, seed=U.IMG_SEED)[0].double()
    _, order = relu_inputs(model, img)
    # 'sub' runs a subset of the ReLUs of 'max' in the same order; order them as 'max' does
    moved = {}
    for key in order:
        by_name, _ = relu_inputs(model, img)     # everything upstream of `key` is final by now
        bias = params[key]
        for c in range(bias.numel()):
            cols = [(v[:, c], rms) for v, rms in by_name[key] if v.shape[1] > c]
            base = float(bias[c])
            for k in range(200):
                shift = ((k + 1) // 2) * STEP * cols[0][1] * (1 if k % 2 else -1)
                new = torch.tensor(base + shift, dtype=torch.float32)
                delta = float(new) - base
                if all(float((v + delta).abs().min()) >= TARGET * rms for v, rms in cols):
                    break
            else:
                raise AssertionError("%s[%d]: no shift clears the margin" % (key, c))
            if k:
                with torch.no_grad():
                    bias[c] = new
                moved.setdefault(key, []).append([c, repr(float(new))])
        print("%-50s %3d of %3d channels moved" % (key, len(moved.get(key, [])), bias.numel()), flush=True)
    by_name, _ = relu_inputs(model, img)
    worst = min(float(v.abs().min()) / rms for vs in by_name.values() for v, rms in vs)
    assert worst >= 1.1e-4, worst
    path = os.path.join(HERE, "convformer_relu_margin.json")
    with open(path, "w") as f:
        json.dump(dict(seed=U.SEED, img_seed=U.IMG_SEED, margin=worst, bias=moved), f, indent=1, sort_keys=True)
    print("wrote %s: %d values, smallest |input| / rms %.3g" % (path, sum(map(len, moved.values())), worst))


if __name__ == "__main__":
    main()
