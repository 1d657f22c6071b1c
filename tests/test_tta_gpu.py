"""Multi-scale / flip test-time augmentation on the GPU: gs_tta_views against the existing
gs_seg_augment test path and the oracle, evaluation through the TTA loader against a manual loop,
gs_seg_overlay against numpy, and the inference API."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util_models import arch_meta, fcn_head, model_cfg, randomize

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
NORM = dict(type="Normalize", mean=list(MEAN), std=list(STD), to_rgb=True)
INNER = [dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"), NORM,
         dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])]
SCALE = (96, 64)
TTA_PIPELINE = [dict(type="LoadImageFromFile"),
                dict(type="MultiScaleFlipAug", img_scale=SCALE, img_ratios=[0.5, 1.0, 1.5], flip=True,
                     transforms=INNER)]
ONE_PIPELINE = [dict(type="LoadImageFromFile"),
                dict(type="MultiScaleFlipAug", img_scale=SCALE, flip=False, transforms=INNER)]
SENTINEL = -12345.0
GUARD = 1024


# ---- 1. the views -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 53), (3, 5)])
@pytest.mark.parametrize("src_is_rgb", [False, True])
@pytest.mark.parametrize("to_rgb", [True, False])
def test_views_equal_the_existing_kernel_mirror_exactly_and_stay_in_their_slots(hip_lib, size, src_is_rgb,
                                                                                to_rgb):
    from gaia_seg_amd.datasets import GpuTrainPipeline
    from gaia_seg_amd.datasets.gpu_pipeline import rescale_size
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    from oracle.pipeline import resize_bilinear_u8
    h, w = size
    rng = np.random.RandomState(h * 100 + w)
    imgs = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(2)]
    samples = [(torch.from_numpy(a), None) for a in imgs]
    pipe = GpuTrainPipeline(mean=MEAN, std=STD, to_rgb=to_rgb, src_is_rgb=src_is_rgb, photometric=False,
                            flip_ratio=0.0)
    scales = [(int(w * r), int(h * r)) for r in (0.5, 1.0, 1.75, 2.0)]
    views = [dict(scale=s, flip=f, flip_direction=d) for s in scales
             for f, d in ((False, "horizontal"), (True, "horizontal"), (True, "vertical"))]
    # direct launches into guarded buffers: one flat buffer per view, sentinel on both sides
    n = len(samples)
    sizes = [rescale_size(h, w, v["scale"]) for v in views]
    bufs = [torch.full((2 * GUARD + n * 3 * rh * rw,), SENTINEL, dtype=torch.float32, device="cuda")
            for rh, rw in sizes]
    d = lib.TtaDesc()
    d.src_h, d.src_w, d.src_is_rgb, d.n_views, d.to_rgb = h, w, int(src_is_rgb), len(views), int(to_rgb)
    for k in range(3):
        d.mean[k], d.std[k] = MEAN[k], STD[k]
    for k, (v, (rh, rw)) in enumerate(zip(views, sizes)):
        d.views[k].res_h, d.views[k].res_w = rh, rw
        d.views[k].flip = lib.FLIP_CODES[v["flip_direction"] if v["flip"] else None]
    for i, s in enumerate(samples):
        src = s[0].cuda().contiguous()
        for k, (rh, rw) in enumerate(sizes):
            d.views[k].out = bufs[k].data_ptr() + 4 * (GUARD + i * 3 * rh * rw)
        lib.check(hip_lib.gs_tta_views(d, src.data_ptr(), current_stream_ptr()), "gs_tta_views")
    torch.cuda.synchronize()
    got = []
    for buf, (rh, rw) in zip(bufs, sizes):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
        got.append(buf[GUARD:-GUARD].view(n, 3, rh, rw))
    assert not any(bool((g == SENTINEL).any()) for g in got)        # every slot fully written
    for k in range(0, len(views), 3):
        rh, rw = sizes[k]
        plain = got[k]
        want = pipe.test_batch(samples, views[k]["scale"])["img"]   # gs_seg_augment at that scale
        assert tuple(want.shape) == (n, 3, rh, rw)
        assert torch.equal(plain, want)
        assert torch.equal(got[k + 1], plain.flip(-1))
        assert torch.equal(got[k + 2], plain.flip(-2))
        for i, a in enumerate(imgs):
            bgr = a[:, :, ::-1] if src_is_rgb else a
            im = resize_bilinear_u8(bgr, rh, rw)
            if to_rgb:
                im = im[..., ::-1]
            ref = ((im.astype(np.float32) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32))
            diff = np.abs(plain[i].cpu().numpy() - ref.transpose(2, 0, 1))
            # the tolerance of tests/test_pipeline_gpu.py for gs_seg_augment: the same fp32
            # operations in the same order, equal up to the last bit of the final division
            assert float(diff.max()) <= 1e-6, (views[k], float(diff.max()))
    # the pipeline's own entry point gives the same tensors and the metas of test_batch
    batch = pipe.tta_batch(samples, views)
    assert len(batch["img"]) == len(views) and "gt_semantic_seg" not in batch
    for k, v in enumerate(views):
        assert torch.equal(batch["img"][k], got[k])
        m = batch["img_metas"][k]
        base = pipe.test_batch(samples, v["scale"])["img_metas"]
        assert len(m) == n and set(m[0]) == set(base[0])
        for a, b in zip(m, base):
            assert a == dict(b, flip=v["flip"], flip_direction=v["flip_direction"])


# ---- shared model and data ----------------------------------------------------------------------
def _write_dataset(root):
    """Three 32 x 48 images and one of 40 x 48 (sorted last), blocky so that predictions vary."""
    from PIL import Image
    rng = np.random.RandomState(7)
    os.makedirs(os.path.join(root, "img"))
    os.makedirs(os.path.join(root, "ann"))
    for name, (h, w) in (("a", (32, 48)), ("b", (32, 48)), ("c", (32, 48)), ("d", (40, 48))):
        base = rng.randint(0, 256, size=(h // 8, w // 8, 3)).astype(np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))
        img[rng.rand(h, w) < 0.2] = rng.randint(0, 256, size=3)
        lab = np.kron(rng.randint(0, 19, size=(h // 4, w // 4)).astype(np.uint8), np.ones((4, 4), np.uint8))
        lab[rng.rand(h, w) < 0.05] = 255
        Image.fromarray(img, "RGB").save(os.path.join(root, "img", name + ".png"))
        Image.fromarray(lab, "L").save(os.path.join(root, "ann", name + ".png"))


def _dataset_cfg(root, pipeline):
    return dict(type="CustomDataset", img_dir=os.path.join(root, "img"), ann_dir=os.path.join(root, "ann"),
                img_suffix=".png", seg_map_suffix=".png", pipeline=pipeline)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gaia_seg_amd.datasets import GpuTrainPipeline, build_dataset
    from gaia_seg_amd.models import build_segmentor
    root = str(tmp_path_factory.mktemp("tta"))
    _write_dataset(root)
    cfg = model_cfg(fcn_head(), aux=True)
    model = build_segmentor(copy.deepcopy(cfg))
    randomize(model, 3)
    model = model.cuda().eval()
    model.manipulate_arch(arch_meta("sub"))
    ds = build_dataset(_dataset_cfg(root, TTA_PIPELINE))
    pipe = GpuTrainPipeline(mean=MEAN, std=STD, to_rgb=True, src_is_rgb=True, photometric=False,
                            flip_ratio=0.0)
    return dict(root=root, cfg=cfg, model=model, ds=ds, pipe=pipe)


def _manual_views(pipe, samples, kw):
    """Every view built the way the parent commit can: test_batch at the scale plus torch.flip."""
    from gaia_seg_amd.datasets import tta_views
    h, w = samples[0][0].shape[:2]
    imgs, metas = [], []
    for v in tta_views(kw, h, w):
        b = pipe.test_batch(samples, v["scale"])
        img = b["img"]
        if v["flip"]:
            img = img.flip(-1 if v["flip_direction"] == "horizontal" else -2).contiguous()
        imgs.append(img)
        metas.append([dict(m, flip=v["flip"], flip_direction=v["flip_direction"]) for m in b["img_metas"]])
    return imgs, metas


def _manual_metrics(model, ds, pipe, kw, groups):
    from gaia_seg_amd.core.evaluation import metrics_from_confusion
    conf = np.zeros((19, 19), dtype=np.int64)
    for group in groups:
        samples = [ds.read(i) for i in group]
        imgs, metas = _manual_views(pipe, samples, kw)
        with torch.no_grad():
            preds = model.aug_test(imgs, metas)
        for pred, s in zip(preds, samples):
            lab = s[1].numpy().astype(np.int64)
            m = lab != 255
            np.add.at(conf, (lab[m], pred[m]), 1)
    # on the device, as evaluate_model reduces it: the same sums in the same order
    return metrics_from_confusion(torch.from_numpy(conf).cuda())


GROUPS = [[0, 1], [2], [3]]       # batches of two hold samples of one size


# ---- 2. evaluation end to end -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["whole", "slide"])
def test_evaluate_model_over_the_tta_loader_equals_a_manual_loop(hip_lib, world, mode):
    from gaia_seg_amd.apis.train import build_dataloader
    from gaia_seg_amd.core.config import ConfigDict
    from gaia_seg_amd.core.evaluation import evaluate_model
    from gaia_seg_amd.datasets import FileTtaEvalLoader, tta_pipeline_kwargs
    model, ds, pipe = world["model"], world["ds"], world["pipe"]
    saved = model.test_cfg
    model.test_cfg = ConfigDict(dict(mode="whole") if mode == "whole" else
                                dict(mode="slide", crop_size=(24, 24), stride=(16, 16)))
    try:
        loader = build_dataloader(_dataset_cfg(world["root"], TTA_PIPELINE), 2, device="cuda", train=False)
        assert isinstance(loader, FileTtaEvalLoader) and len(loader) == 2
        got = evaluate_model(model, loader, len(GROUPS), 19)
        loader.close()
        want = _manual_metrics(model, ds, pipe, tta_pipeline_kwargs(TTA_PIPELINE), GROUPS)
        print("tta %s: mIoU %.6f mAcc %.6f aAcc %.6f" % (mode, got["mIoU"], got["mAcc"], got["aAcc"]))
        np.testing.assert_equal(got, want)          # bit-identical views: exact (NaN == NaN)
        if mode == "whole":
            # guards against silently evaluating one view
            one = build_dataloader(_dataset_cfg(world["root"], ONE_PIPELINE), 2, device="cuda", train=False)
            assert not isinstance(one, FileTtaEvalLoader)
            single = evaluate_model(model, one, len(GROUPS), 19)
            one.close()
            print("single view: mIoU %.6f" % single["mIoU"])
            assert single["mIoU"] != got["mIoU"]
    finally:
        model.test_cfg = saved


# ---- 3. aug_test_device -------------------------------------------------------------------------
def test_aug_test_device_equals_aug_test(hip_lib, world):
    from gaia_seg_amd.datasets import tta_pipeline_kwargs, tta_views
    model, ds, pipe = world["model"], world["ds"], world["pipe"]
    samples = [ds.read(0), ds.read(1)]
    batch = pipe.tta_batch(samples, tta_views(tta_pipeline_kwargs(TTA_PIPELINE), 32, 48))
    assert tuple(batch["gt_semantic_seg"].shape) == (2, 1, 32, 48)
    with torch.no_grad():
        dev = model.aug_test_device(batch["img"], batch["img_metas"])
        host = model.aug_test(batch["img"], batch["img_metas"])
    assert dev.is_cuda and dev.dtype == torch.int64 and tuple(dev.shape) == (2, 32, 48)
    assert len(host) == 2 and np.array_equal(np.stack(host), dev.cpu().numpy())


# ---- 4. overlay ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 7), (33, 65)])
@pytest.mark.parametrize("opacity", [0.5, 0.3])
def test_overlay_equals_numpy_exactly(hip_lib, size, opacity):
    from gaia_seg_amd.core.visual import overlay
    from gaia_seg_amd.datasets.custom import _CITYSCAPES_PALETTE
    h, w = size
    rng = np.random.RandomState(h + w)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    seg = rng.randint(0, 19, size=(h, w)).astype(np.int64)
    seg[rng.rand(h, w) < 0.1] = 255
    seg[0, 0], seg[-1, -1] = 255, -1
    palette = np.array(_CITYSCAPES_PALETTE)
    color_seg = np.zeros((h, w, 3), dtype=np.uint8)
    for label, color in enumerate(palette):
        color_seg[seg == label, :] = color
    color_seg = color_seg[..., ::-1]
    want = (img * (1 - opacity) + color_seg * opacity).astype(np.uint8)
    got = overlay(seg, img, palette, opacity)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(overlay(torch.from_numpy(seg).cuda(), img, palette, opacity), want)


# ---- 5. inference API ---------------------------------------------------------------------------
def _write_config(path, model, pipeline):
    with open(path, "w") as f:
        f.write("model = %r\n" % (model,))
        f.write("data = dict(test=dict(type='CustomDataset', img_dir='.', pipeline=%r))\n" % (pipeline,))


def test_inference_api_and_demo_tool(hip_lib, world, tmp_path):
    from gaia_seg_amd.apis import inference_segmentor, init_segmentor
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.datasets import tta_pipeline_kwargs
    from gaia_seg_amd.datasets.custom import _CITYSCAPES_CLASSES, _CITYSCAPES_PALETTE
    model, ds, pipe = world["model"], world["ds"], world["pipe"]
    ck = str(tmp_path / "supernet.pth")
    save_checkpoint(model, ck, meta=dict(CLASSES=_CITYSCAPES_CLASSES, PALETTE=_CITYSCAPES_PALETTE))
    png = ds.image_path(3)                                   # the 40 x 48 image
    sample = ds.read(3)
    # single view == simple_test on test_batch of the same image
    one_cfg = str(tmp_path / "one.py")
    _write_config(one_cfg, world["cfg"], ONE_PIPELINE)
    net = init_segmentor(one_cfg, ck, arch=arch_meta("sub"))
    assert net.CLASSES == _CITYSCAPES_CLASSES and not net.training and net.cfg.data.test.pipeline
    got = inference_segmentor(net, png)
    b = pipe.test_batch([sample], SCALE)
    with torch.no_grad():
        want = model.simple_test(b["img"], b["img_metas"])
    assert len(got) == 1 and got[0].shape == (40, 48) and np.array_equal(got[0], want[0])
    # a BGR array is the same picture
    bgr = np.ascontiguousarray(sample[0].numpy()[:, :, ::-1])
    assert np.array_equal(inference_segmentor(net, bgr)[0], want[0])
    # the TTA pipeline == the manual loop over its views
    tta_cfg = str(tmp_path / "tta.py")
    _write_config(tta_cfg, world["cfg"], TTA_PIPELINE)
    net = init_segmentor(tta_cfg, ck, arch=arch_meta("sub"))
    got = inference_segmentor(net, [png, ds.image_path(0)])
    kw = tta_pipeline_kwargs(TTA_PIPELINE)
    for k, idx in enumerate((3, 0)):
        imgs, metas = _manual_views(pipe, [ds.read(idx)], kw)
        with torch.no_grad():
            want = model.aug_test(imgs, metas)
        assert np.array_equal(got[k], want[0])
    # show_result: a file of the image's size holding the returned blend
    from PIL import Image
    out = str(tmp_path / "shown.png")
    blend = net.show_result(png, got[:1], opacity=0.5, out_file=out)
    with Image.open(out) as im:
        assert im.size == (48, 40)
        assert np.array_equal(np.array(im.convert("RGB"))[:, :, ::-1], blend)
    # the command-line tool, in a process of its own
    demo_out = str(tmp_path / "demo.png")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "demo_image.py"), png, tta_cfg, ck, "--arch",
           '{"arch.backbone.stem.width": 16, "arch.backbone.body.width": [16, 48, 64, 96], '
           '"arch.backbone.body.depth": [1, 2, 2, 1]}', "--out", demo_out, "--opacity", "0.3"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    with Image.open(demo_out) as im:
        assert im.size == (48, 40)
        want = net.show_result(png, got[:1], opacity=0.3)
        assert np.array_equal(np.array(im.convert("RGB"))[:, :, ::-1], want)


# ---- 6. TTA does not compose with apply_input_shape ----------------------------------------------
def test_tta_with_apply_input_shape_raises_at_set_up(hip_lib, world):
    from gaia_seg_amd.apis.test import test_model_space as run_model_space
    from gaia_seg_amd.apis.train import build_dataloader
    from gaia_seg_amd.core.evaluation import CrossArchEvalHook, evaluate_model
    loader = build_dataloader(_dataset_cfg(world["root"], TTA_PIPELINE), 2, device="cuda", train=False)
    try:
        with pytest.raises(ValueError, match="apply_input_shape"):
            CrossArchEvalHook(loader, None, apply_input_shape=True)
        meta = {"name": "sub", "arch.backbone.stem.width": 16, "arch.backbone.body.width": [16, 48, 64, 96],
                "arch.backbone.body.depth": [1, 2, 2, 1], "data.input_shape": 32}
        with pytest.raises(ValueError, match="apply_input_shape"):
            run_model_space(world["model"], loader, [meta], 1, 19, apply_input_shape=True)
        with pytest.raises(ValueError, match="apply_input_shape"):
            evaluate_model(world["model"], loader, 1, 19, input_shape=32)
    finally:
        loader.close()
