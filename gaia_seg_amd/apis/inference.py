"""Inference on images -- host-side mirror of gaiaseg/apis/inference.py:23-128 (init_segmentor,
inference_segmentor, show_result_pyplot).

What differs by design: the test pipeline of ``cfg.data.test`` is not composed from CPU transforms;
it is translated into a list of views (datasets.custom.tta_pipeline_kwargs) that one ``gs_tta_views``
launch per image produces on the device, and files are decoded with Pillow.  A supernet checkpoint
needs to be told which subnet to run (``arch`` or ``cfg.model_sampler``); a checkpoint written by
tools/extract_subnet.py, loaded into a config of its own size, needs nothing."""
import numpy as np
import torch

from ..core.checkpoint import load_checkpoint
from ..core.config import Config
from ..core.dynamic import fold_dict
from ..core.model_space import _listify, build_model_sampler
from ..datasets.custom import tta_pipeline_kwargs, tta_views
from ..datasets.gpu_pipeline import GpuTrainPipeline
from ..models import build_segmentor


def _anchors(cfg):
    out = []
    for key in ("model_sampler", "val_sampler", "train_sampler"):
        if cfg.get(key):
            sampler = build_model_sampler(cfg[key])
            sampler.set_mode("traverse")
            out.extend(sampler.traverse())
    return out


def resolve_arch(cfg, arch=None):
    """The folded arch dict ``manipulate_arch`` takes, or None (run the model as built).  ``arch``: a
    flat meta (``arch.backbone...`` keys), a folded dict (``{'backbone': ...}``) or the name of an
    anchor of ``cfg.model_sampler`` / ``val_sampler`` / ``train_sampler``; without it the first
    subnet of ``cfg.model_sampler`` when the config has one."""
    if arch is None:
        if not cfg.get("model_sampler"):
            return None
        sampler = build_model_sampler(cfg.model_sampler)
        sampler.set_mode("traverse")
        arch = sampler.traverse()[0]
    if isinstance(arch, str):
        named = [m for m in _anchors(cfg) if m.get("name") == arch]
        if not named:
            raise KeyError("no anchor named %r in the config's model samplers" % (arch,))
        arch = named[0]
    arch = dict(arch)
    if any(k.startswith("arch.") for k in arch):
        arch = fold_dict(arch)["arch"]
    elif "arch" in arch:
        arch = arch["arch"]
    return _listify(arch)


def init_segmentor(config, checkpoint=None, device="cuda:0", arch=None):
    """Build the segmentor of ``config`` (a path or a Config), load ``checkpoint`` and its
    ``meta['CLASSES']`` / ``meta['PALETTE']`` when present, select the subnet (``resolve_arch``), keep
    the config as ``model.cfg`` and switch to eval mode."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError("config must be a filename or Config object, but got %s" % type(config))
    config.model.pretrained = None
    model = build_segmentor(config.model, train_cfg=config.get("train_cfg"),
                            test_cfg=config.get("test_cfg"))
    if checkpoint is not None:
        ck = load_checkpoint(model, checkpoint, map_location="cpu")
        meta = ck.get("meta") or {}
        if meta.get("CLASSES") is not None:
            model.CLASSES = meta["CLASSES"]
        if meta.get("PALETTE") is not None:
            model.PALETTE = meta["PALETTE"]
    model.cfg = config
    model.to(device)
    model.eval()
    folded = resolve_arch(config, arch)
    if folded is not None:
        model.manipulate_arch(folded)
    return model


def _decode(img):
    """(uint8 host tensor [H, W, 3], is it RGB?, file name)"""
    if isinstance(img, str):
        from PIL import Image
        with Image.open(img) as im:
            return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)), True, img
    arr = np.ascontiguousarray(img)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise TypeError("expected a file path or a uint8 BGR array [H, W, 3]")
    return torch.from_numpy(arr), False, None


def inference_segmentor(model, img):
    """Label maps (list of int64 arrays at the images' own sizes) for a file path, a uint8 BGR array
    or a list of them, through ``cfg.data.test.pipeline`` -- every view of its MultiScaleFlipAug --
    and ``forward_test``."""
    cfg = model.cfg
    device = next(model.parameters()).device
    kw = tta_pipeline_kwargs(cfg.data.test.pipeline)
    results = []
    for one in (img if isinstance(img, (list, tuple)) else [img]):
        pixels, is_rgb, name = _decode(one)
        pipe = GpuTrainPipeline(mean=kw["mean"], std=kw["std"], to_rgb=kw["to_rgb"], device=device,
                                src_is_rgb=is_rgb, photometric=False, flip_ratio=0.0)
        h, w = int(pixels.shape[0]), int(pixels.shape[1])
        batch = pipe.tta_batch([(pixels, None, name or "array")], tta_views(kw, h, w))
        with torch.no_grad():
            results.extend(model(return_loss=False, rescale=True, img=batch["img"],
                                 img_metas=batch["img_metas"]))
    return results


def show_result_pyplot(model, img, result, palette=None, fig_size=(15, 10), opacity=0.5):
    """The blended image in a matplotlib figure (needs matplotlib)."""
    import matplotlib.pyplot as plt
    img = model.show_result(img, result, palette=palette, opacity=opacity)
    plt.figure(figsize=fig_size)
    plt.imshow(img[:, :, ::-1])
    plt.show()
