"""Multi-scale / flip test-time augmentation, host side: the view list of a MultiScaleFlipAug test
pipeline, its refusals, and the argument checks of gs_tta_views / gs_seg_overlay (no GPU)."""
import ctypes

import pytest

from gaia_seg_amd.datasets import (eval_pipeline_kwargs, tta_num_views, tta_pipeline_kwargs,
                                   tta_views)
from gaia_seg_amd.hip import lib

NORM = dict(type="Normalize", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


def pipeline(inner=None, **aug):
    inner = inner if inner is not None else [dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"),
                                             NORM, dict(type="ImageToTensor", keys=["img"]),
                                             dict(type="Collect", keys=["img"])]
    aug.setdefault("img_scale", (2048, 1024))
    return [dict(type="LoadImageFromFile"), dict(type="MultiScaleFlipAug", transforms=inner, **aug)]


def test_six_ratios_with_flip_give_twelve_views():
    kw = tta_pipeline_kwargs(pipeline(img_ratios=RATIOS, flip=True))
    assert tta_num_views(kw) == 12
    views = tta_views(kw, 1024, 2048)
    assert len(views) == 12
    assert [v["scale"] for v in views[::2]] == [(1024, 512), (1536, 768), (2048, 1024), (2560, 1280),
                                                (3072, 1536), (3584, 1792)]
    assert [v["scale"] for v in views[1::2]] == [v["scale"] for v in views[::2]]
    assert [v["flip"] for v in views] == [False, True] * 6
    assert {v["flip_direction"] for v in views} == {"horizontal"}
    assert (kw["mean"], kw["std"], kw["to_rgb"]) == ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375), True)
    # a fixed ladder does not depend on the image
    assert tta_views(kw, 37, 53) == views


def test_ratios_without_a_scale_follow_each_image():
    kw = tta_pipeline_kwargs(pipeline(img_scale=None, img_ratios=RATIOS, flip=False))
    views = tta_views(kw, 37, 53)
    assert [v["scale"] for v in views] == [(int(53 * r), int(37 * r)) for r in RATIOS]
    assert [v["scale"] for v in views][:2] == [(26, 18), (39, 27)]
    assert not any(v["flip"] for v in views)
    with pytest.raises(ValueError):
        tta_pipeline_kwargs(pipeline(img_scale=None))


def test_a_list_of_scales_is_taken_as_given():
    kw = tta_pipeline_kwargs(pipeline(img_scale=[(512, 256), (1024, 512)], flip=True))
    assert [(v["scale"], v["flip"]) for v in tta_views(kw, 10, 20)] == [
        ((512, 256), False), ((512, 256), True), ((1024, 512), False), ((1024, 512), True)]


def test_two_directions_repeat_the_unflipped_view():
    kw = tta_pipeline_kwargs(pipeline(img_ratios=[0.5, 1.0], flip=True,
                                      flip_direction=["horizontal", "vertical"]))
    views = tta_views(kw, 8, 16)
    assert len(views) == 8
    per_scale = [(v["flip"], v["flip_direction"]) for v in views[:4]]
    assert per_scale == [(False, "horizontal"), (False, "vertical"), (True, "horizontal"), (True, "vertical")]
    assert [(v["flip"], v["flip_direction"]) for v in views[4:]] == per_scale
    assert {v["scale"] for v in views[:4]} == {(1024, 512)} and {v["scale"] for v in views[4:]} == {(2048, 1024)}
    one = tta_pipeline_kwargs(pipeline(flip=True, flip_direction="vertical"))
    assert [(v["flip"], v["flip_direction"]) for v in tta_views(one, 8, 16)] == [(False, "vertical"),
                                                                                (True, "vertical")]


def test_a_single_view_list_yields_one_unflipped_view():
    kw = tta_pipeline_kwargs(pipeline(flip=False))
    assert tta_num_views(kw) == 1
    assert tta_views(kw, 5, 9) == [dict(scale=(2048, 1024), flip=False, flip_direction="horizontal")]


@pytest.mark.parametrize("inner", [
    [dict(type="Resize", keep_ratio=False), NORM],
    [dict(type="Resize", keep_ratio=True), dict(type="Pad", size_divisor=32), NORM],
    [dict(type="ResizeToMultiple", size_divisor=32), NORM],
    [dict(type="Resize", keep_ratio=True), dict(type="PhotoMetricDistortion"), NORM],
])
def test_inner_transforms_without_a_counterpart_are_refused(inner):
    with pytest.raises(NotImplementedError):
        tta_pipeline_kwargs(pipeline(inner=inner, img_ratios=RATIOS, flip=True))


def test_other_refusals():
    with pytest.raises(NotImplementedError):       # 18 views
        tta_pipeline_kwargs(pipeline(img_ratios=[0.5 + 0.125 * k for k in range(9)], flip=True))
    tta_pipeline_kwargs(pipeline(img_ratios=[0.5 + 0.125 * k for k in range(8)], flip=True))   # 16: fine
    with pytest.raises(NotImplementedError):
        tta_pipeline_kwargs(pipeline(flip=True, flip_direction="diagonal"))
    with pytest.raises(NotImplementedError):
        tta_pipeline_kwargs(pipeline(flip=True) + [dict(type="RandomCrop", crop_size=(8, 8))])
    with pytest.raises(ValueError):
        tta_pipeline_kwargs([dict(type="LoadImageFromFile"), NORM])
    # the single-view translation keeps refusing what it refused
    with pytest.raises(NotImplementedError):
        eval_pipeline_kwargs(pipeline(img_ratios=RATIOS, flip=True))


def test_loader_choice_follows_the_pipeline():
    from gaia_seg_amd.apis.train import wants_tta
    assert wants_tta(pipeline(img_ratios=RATIOS, flip=True))
    assert wants_tta(pipeline(flip=True)) and wants_tta(pipeline(img_scale=None, img_ratios=[1.0]))
    assert not wants_tta(pipeline(flip=False))
    assert not wants_tta([dict(type="LoadImageFromFile"), NORM])


def test_tta_with_apply_input_shape_is_refused_at_set_up():
    from gaia_seg_amd.core.evaluation import CrossArchEvalHook, check_tta_input_shape, is_tta_loader

    class Loader:
        tta = True
    views = [dict(img=[None, None], img_metas=[[], []])]
    assert is_tta_loader(Loader()) and is_tta_loader(views)
    assert not is_tta_loader([dict(img=None, img_metas=[])]) and not is_tta_loader(object())
    for loader in (Loader(), views):
        with pytest.raises(ValueError, match="apply_input_shape"):
            check_tta_input_shape(loader, True)
        with pytest.raises(ValueError, match="apply_input_shape"):
            CrossArchEvalHook(loader, None, apply_input_shape=True)
        check_tta_input_shape(loader, False)
        CrossArchEvalHook(loader, None, apply_input_shape=False)
    CrossArchEvalHook([dict(img=None)], None, apply_input_shape=True)


# ---- C ABI: argument checks happen before any launch, so they need no device --------------------
def _desc(n_views=1, res=(4, 6), flip=0, out=64):
    d = lib.TtaDesc()
    d.src_h, d.src_w, d.n_views, d.to_rgb = 5, 7, n_views, 1
    for k in range(3):
        d.mean[k], d.std[k] = 0.0, 1.0
    for k in range(max(0, min(n_views, lib.TTA_MAX_VIEWS))):
        d.views[k].res_h, d.views[k].res_w, d.views[k].flip, d.views[k].out = res[0], res[1], flip, out
    return d


def test_tta_views_argument_validation_needs_no_gpu():
    L = lib.load()
    assert ctypes.sizeof(lib.TtaView) == 24
    assert ctypes.sizeof(lib.TtaDesc) == 12 * 4 + 16 * 24
    img = 64      # never dereferenced: every call below is refused before a launch
    assert L.gs_tta_views(_desc(), None, None) == -4
    assert L.gs_tta_views(_desc(out=None), img, None) == -4
    for bad in (_desc(n_views=0), _desc(n_views=17), _desc(n_views=-1), _desc(res=(0, 6)),
                _desc(res=(4, -1)), _desc(flip=3), _desc(flip=-1)):
        assert L.gs_tta_views(bad, img, None) == -1
    d = _desc(n_views=2)
    d.views[1].flip = 5
    assert L.gs_tta_views(d, img, None) == -1
    d = _desc()
    d.src_h = 0
    assert L.gs_tta_views(d, img, None) == -1
    d = _desc()
    d.std[1] = 0.0
    assert L.gs_tta_views(d, img, None) == -1


def test_seg_overlay_argument_validation_needs_no_gpu():
    L = lib.load()
    p = 64
    assert L.gs_seg_overlay(None, p, p, 19, 4, 4, 0.5, p, None) == -4
    assert L.gs_seg_overlay(p, None, p, 19, 4, 4, 0.5, p, None) == -4
    assert L.gs_seg_overlay(p, p, None, 19, 4, 4, 0.5, p, None) == -4
    assert L.gs_seg_overlay(p, p, p, 19, 4, 4, 0.5, None, None) == -4
    assert L.gs_seg_overlay(p, p, p, 0, 4, 4, 0.5, p, None) == -1
    assert L.gs_seg_overlay(p, p, p, 19, 0, 4, 0.5, p, None) == -1
    assert L.gs_seg_overlay(p, p, p, 19, 4, -2, 0.5, p, None) == -1
    assert L.gs_seg_overlay(p, p, p, 19, 4, 4, 1.5, p, None) == -1
    assert L.gs_seg_overlay(p, p, p, 19, 4, 4, -0.1, p, None) == -1
    assert L.gs_seg_overlay(p, p, p, 19, 4, 4, float("nan"), p, None) == -1
