"""Elastic input resolution, host side: the ``data.input_shape`` parser, the
refusals, the argument checks of gs_batch_rescale (no launch is made) and tools/count_flops.py
--apply-input-shape.  Nothing here needs a GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resolve_input_shape_forms():
    from gaia_seg_amd.core.model_space import resolve_input_shape as r
    # int S: the short side becomes S, the long side floor(S * long / short + 0.5)
    assert r(48, 64, 96) == (48, 72)
    assert r(48, 96, 64) == (72, 48)              # portrait: the short side is the width
    assert r(800, 512, 1024) == (800, 1600)
    assert r(50, 64, 64) == (50, 50)
    # rounding of the long side: 51 * 96 / 64 = 76.5 -> 77 (half rounds up), 33 * 100 / 64 = 51.56 -> 52,
    # 35 * 100 / 64 = 54.69 -> 55, 45 * 97 / 64 = 68.2 -> 68
    assert r(51, 64, 96) == (51, 77)
    assert r(33, 64, 100) == (33, 52)
    assert r(35, 64, 100) == (35, 55)
    assert r(45, 64, 97) == (45, 68)
    # sequences and the string form: exactly the last two entries, the aspect ratio is not kept
    assert r((56, 100), 64, 96) == (56, 100)
    assert r([56, 100], 64, 96) == (56, 100)
    assert r((3, 800, 800), 512, 1024) == (800, 800)
    assert r("3,800,800", 512, 1024) == (800, 800)
    assert r("56, 100", 64, 96) == (56, 100)
    # a target equal to the batch size is the batch size (the caller passes the batch through)
    assert r(64, 64, 96) == (64, 96)
    assert r((64, 96), 64, 96) == (64, 96)
    assert r("3,64,96", 64, 96) == (64, 96)


@pytest.mark.parametrize("bad", [0, -480, 1.5, 480.0, True, None, (0, 100), (56, -1), (1, 800, 800),
                                 (4, 800, 800), (3, 0, 800), (800,), (3, 3, 800, 800), (), "800",
                                 "1,800,800", "3,800,x", "", {"h": 1}, (56.0, 100)])
def test_resolve_input_shape_refuses(bad):
    from gaia_seg_amd.core.model_space import parse_input_shape, resolve_input_shape
    with pytest.raises(ValueError):
        resolve_input_shape(bad, 64, 96)
    with pytest.raises(ValueError):
        parse_input_shape(bad)


def test_flag_with_distillation_is_refused_at_setup():
    from gaia_seg_amd.apis.train import check_input_shape_cfg
    from gaia_seg_amd.core.config import Config
    assert check_input_shape_cfg(Config(dict())) is False
    assert check_input_shape_cfg(Config(dict(apply_input_shape=True))) is True
    assert check_input_shape_cfg(Config(dict(use_distillation=True))) is False
    with pytest.raises(ValueError, match="use_distillation"):
        check_input_shape_cfg(Config(dict(apply_input_shape=True, use_distillation=True)))
    # the hook refuses as well (a runner assembled by hand)
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import SandwichHook
    import types
    hook = SandwichHook(build_model_sampler(dict(type="concat", model_samplers=[])))
    import gaia_seg_amd.core.runner as R
    keep = R.check_sandwich_model
    R.check_sandwich_model = lambda model: None
    try:
        hook.before_run(types.SimpleNamespace(model=None, apply_input_shape=False))
        with pytest.raises(ValueError, match="use_distillation"):
            hook.before_run(types.SimpleNamespace(model=None, apply_input_shape=True))
    finally:
        R.check_sandwich_model = keep


def test_bad_row_values_are_refused_before_any_work():
    """finetune's set-up check and test_model_space refuse a bad value before touching the model."""
    from gaia_seg_amd.apis.finetune import check_finetune_cfg
    from gaia_seg_amd.apis.test import test_model_space
    from gaia_seg_amd.core.config import Config
    base = dict(optimizer=dict(type="SGD", lr=0.01), optimizer_config=dict(),
                lr_config=dict(policy="fixed"))
    rows = [{"name": "a", "data.input_shape": 48}, {"name": "b", "data.input_shape": (1, 48, 48)}]
    check_finetune_cfg(Config(base), rows)                       # flag off: carried, not looked at
    with pytest.raises(ValueError, match="C must be 3"):
        check_finetune_cfg(Config(dict(base, apply_input_shape=True)), rows)
    with pytest.raises(ValueError, match="C must be 3"):
        test_model_space(None, [], rows, 1, 19, apply_input_shape=True)


def test_ranking_reads_the_top_level_key_of_the_models_config():
    """tools/test_supernet.py hands test_model_space the model and no flag: the top-level
    apply_input_shape of the config the model was built from decides (model.top_cfg)."""
    from gaia_seg_amd.apis.test import test_model_space
    from gaia_seg_amd.core.config import Config, DictAction
    from gaia_seg_amd.models import build_segmentor
    from util_models import fcn_head, model_cfg
    rows = [{"name": "b", "data.input_shape": (1, 48, 48)}]
    mc = model_cfg(fcn_head(), aux=True)

    def built(cfg):
        return build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))

    on = Config(dict(model=mc, apply_input_shape=True))
    assert built(on).top_cfg.get("apply_input_shape") is True
    with pytest.raises(ValueError, match="C must be 3"):      # the flag arrived: the bad row is refused
        test_model_space(built(on), [], rows, 1, 19)
    # --cfg-options reach it as well, in both directions
    off = Config(dict(model=mc))
    assert not built(off).top_cfg.get("apply_input_shape", False)
    off.merge_from_dict(DictAction.parse(["apply_input_shape=True"]))
    with pytest.raises(ValueError, match="C must be 3"):
        test_model_space(built(off), [], rows, 1, 19)
    on.merge_from_dict(DictAction.parse(["apply_input_shape=False"]))
    assert built(on).top_cfg.get("apply_input_shape") is False
    # a model built from a plain dict has no config: the key is carried, not applied
    assert build_segmentor(dict(mc)).top_cfg is None
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_elastic_scale.py"))
    assert cfg.apply_input_shape is True and "apply_input_shape" not in cfg.test_cfg
    assert cfg.model._root.get("apply_input_shape") is True and "_root" not in cfg.model


def test_batch_rescale_argument_codes(hip_lib):
    """NULL -> -4, bad sizes -> -1, misalignment -> -2; refused calls launch nothing."""
    L = hip_lib
    a = 0x1000                     # any 16-byte aligned non-null address
    f = L.gs_batch_rescale
    assert f(None, a, 2, 8, 8, a, a, 4, 4, None) == -4
    assert f(a, a, 2, 8, 8, None, a, 4, 4, None) == -4
    assert f(a, a, 2, 8, 8, a, None, 4, 4, None) == -4           # a label without a place to put it
    assert f(a, None, 2, 8, 8, a, a, 4, 4, None) == -4           # ... and the other way round
    for bad in range(5):
        sizes = [2, 8, 8, 4, 4]
        for v in (0, -3):
            sizes[bad] = v
            n, h, w, H, W = sizes
            assert f(a, a, n, h, w, a, a, H, W, None) == -1, sizes
            assert f(a, None, n, h, w, a, None, H, W, None) == -1, sizes
    assert f(a, a, 1, 65536, 65536, a, a, 4, 4, None) == -1       # a plane of 2^32 pixels
    assert f(a, a, 1, 4, 4, a, a, 65536, 65536, None) == -1
    assert f(a, a, 2 ** 31 - 1, 4, 4, a, a, 46340, 46340, None) == -1   # 2^63 output elements and more
    assert f(a, a, 2 ** 31 - 1, 46340, 46340, a, a, 4, 4, None) == -1   # ... and source elements
    assert f(a, a, 2, 8, 8, a + 4, a, 4, 4, None) == -2
    assert f(a, a, 2, 8, 8, a + 8, a, 4, 4, None) == -2
    assert f(a, a, 2, 8, 8, a, a + 8, 4, 4, None) == -2
    assert f(a + 2, a, 2, 8, 8, a, a, 4, 4, None) == -2
    assert f(a, a + 4, 2, 8, 8, a, a, 4, 4, None) == -2
    assert f(a + 2, None, 2, 8, 8, a, None, 4, 4, None) == -2
    from gaia_seg_amd.hip import lib
    assert lib.ABI_VERSION >= 12
    header = open(os.path.join(ROOT, "include", "gaiaseg_hip.h")).read()
    assert "int gs_batch_rescale(" in header


def test_ops_wrapper_refuses_cpu_tensors_and_bad_shapes(hip_lib):
    import torch
    from gaia_seg_amd.hip import lib, ops
    with pytest.raises(lib.HipLibraryError):
        ops.batch_rescale(torch.zeros(1, 3, 4, 4), None, (2, 2))


def test_count_flops_apply_input_shape(tmp_path):
    """Two scales of one arch: different overhead.flops with the option (each the FLOPs at its own
    size), equal without it.  An int keeps --shape's aspect ratio."""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.flops import model_flops
    from gaia_seg_amd.models import build_segmentor
    from util_models import ARCHS, arch_meta, fcn_head, model_cfg
    a = ARCHS["sub"]
    arch = {"arch.backbone.stem.width": a["stem"], "arch.backbone.body.width": a["width"],
            "arch.backbone.body.depth": a["depth"]}
    anchors = [dict(arch, name="s48", **{"data.input_shape": 48}),
               dict(arch, name="s64", **{"data.input_shape": 64}),
               dict(arch, name="e", **{"data.input_shape": "3,56,100"}),
               dict(arch, name="none")]
    cfg_path = os.path.join(str(tmp_path), "cfg.py")
    with open(cfg_path, "w") as fh:
        fh.write("model = %r\nval_sampler = %r\n" % (model_cfg(fcn_head(), aux=True),
                                                      dict(type="anchor", anchors=anchors)))
    tool = _tool("count_flops")
    out_on, out_off = os.path.join(str(tmp_path), "on.json"), os.path.join(str(tmp_path), "off.json")
    tool.main([cfg_path, "--shape", "64", "96", "--out", out_on, "--apply-input-shape"])
    tool.main([cfg_path, "--shape", "64", "96", "--out", out_off])
    on = {r["name"]: r for r in json.load(open(out_on))}
    off = {r["name"]: r for r in json.load(open(out_off))}
    assert len({r["overhead.flops"] for r in off.values()}) == 1
    assert on["s48"]["overhead.flops"] < on["s64"]["overhead.flops"] == off["s64"]["overhead.flops"]
    assert on["none"]["overhead.flops"] == off["none"]["overhead.flops"]
    assert on["s48"]["data.input_shape"] == 48 and on["e"]["data.input_shape"] == "3,56,100"
    assert on["s48"]["overhead.params"] == off["s48"]["overhead.params"]
    model = build_segmentor(Config.fromfile(cfg_path).model)
    model.manipulate_arch(arch_meta("sub"))
    assert on["s48"]["overhead.flops"] == model_flops(model, 48, 72)["total"]
    assert on["e"]["overhead.flops"] == model_flops(model, 56, 100)["total"]
