"""Per-subnet BatchNorm re-calibration, the parts that need no GPU: the ``caliberate_bn.recalibrate``
config key, what refuses it, the C-ABI of the fold launch, and how the calibration loader is built."""
import ctypes
import os
import re

import pytest
import torch

from gaia_seg_amd.core.bn_calibration import build_calibration_batches, parse_recalibrate_cfg
from gaia_seg_amd.core.config import Config
from gaia_seg_amd.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gaiaseg_hip.h")


def test_parse_recalibrate_cfg_values_and_defaults():
    assert parse_recalibrate_cfg(None) is None
    assert parse_recalibrate_cfg({}) is None
    assert parse_recalibrate_cfg(dict(reset_stats=True)) is None
    assert parse_recalibrate_cfg(dict(recalibrate=None)) is None
    assert parse_recalibrate_cfg(dict(recalibrate=None, use_minibatch_stats=True)) is None
    good = dict(recalibrate=dict(num_batches=32, samples_per_gpu=4, seed=7))
    assert parse_recalibrate_cfg(good) == dict(num_batches=32, samples_per_gpu=4, seed=7)
    assert parse_recalibrate_cfg(good, 2) == dict(num_batches=32, samples_per_gpu=4, seed=7)
    # defaults: data.samples_per_gpu and seed 0
    assert parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=3)), 2) == dict(
        num_batches=3, samples_per_gpu=2, seed=0)
    assert parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=3, samples_per_gpu=None)), 2) == dict(
        num_batches=3, samples_per_gpu=2, seed=0)
    # a Config (what the tools pass) reads the same
    cfg = Config(dict(caliberate_bn=dict(recalibrate=dict(num_batches=5)), data=dict(samples_per_gpu=2)))
    assert parse_recalibrate_cfg(cfg.get("caliberate_bn"), cfg.data.get("samples_per_gpu")) == dict(
        num_batches=5, samples_per_gpu=2, seed=0)


def test_parse_recalibrate_cfg_refusals():
    with pytest.raises(KeyError, match="num_batches"):
        parse_recalibrate_cfg(dict(recalibrate=dict(seed=1)))
    for bad in (0, -3, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="num_batches"):
            parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=bad)))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="samples_per_gpu"):
            parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=2, samples_per_gpu=bad)))
    with pytest.raises(ValueError, match="seed"):
        parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=2, seed=0.5)))
    with pytest.raises(KeyError, match="momentum"):
        parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=2, momentum=0.1)))
    with pytest.raises(ValueError, match="use_minibatch_stats"):
        parse_recalibrate_cfg(dict(recalibrate=dict(num_batches=2), use_minibatch_stats=True))


def test_fast_finetune_refuses_recalibrate():
    from gaia_seg_amd.apis.finetune import check_finetune_cfg
    cfg = Config(dict(caliberate_bn=dict(recalibrate=dict(num_batches=2))))
    with pytest.raises(ValueError, match="tools/test_supernet.py"):
        check_finetune_cfg(cfg, [{"name": "a"}])


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_fold_abi_header_binding_and_symbol_agree():
    text = _header_text()
    m = re.search(r"\bint\s+gs_bn_calib_fold\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, "gs_bn_calib_fold is not declared in the header"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = lib.PROTOTYPES["gs_bn_calib_fold"]
    assert nargs == len(args) == 7 and res is ctypes.c_int32
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "gs_bn_calib_fold")
    # the table entry: two pointers + two int32, no padding
    s = re.search(r"typedef struct GsBnCalibLayer \{(.*?)\} GsBnCalibLayer;", text, flags=re.S)
    fields = [f.split()[-1].lstrip("*") for f in s.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in lib.BnCalibLayer._fields_]
    assert ctypes.sizeof(lib.BnCalibLayer) == 24
    assert lib.BnCalibLayer.channels.offset == 16 and lib.BnCalibLayer.offset.offset == 20
    for name, value in (("SAVE", lib.BN_CALIB_SAVE), ("ADD", lib.BN_CALIB_ADD), ("WRITE", lib.BN_CALIB_WRITE)):
        assert re.search(r"#define\s+GS_BN_CALIB_%s\s+%d\b" % (name, value), text), name


def test_fold_argument_checks_need_no_gpu():
    """GS_E_NULL / GS_E_BADARG are returned before any launch."""
    L = lib.load()
    one = ctypes.c_void_p(16)   # never followed: every call below is refused first
    assert L.gs_bn_calib_fold(None, 1, one, 8, lib.BN_CALIB_SAVE, 1.0, None) == -4
    assert L.gs_bn_calib_fold(one, 1, None, 8, lib.BN_CALIB_SAVE, 1.0, None) == -4
    assert L.gs_bn_calib_fold(one, 0, one, 8, lib.BN_CALIB_SAVE, 1.0, None) == -1
    assert L.gs_bn_calib_fold(one, -2, one, 8, lib.BN_CALIB_SAVE, 1.0, None) == -1
    assert L.gs_bn_calib_fold(one, 1, one, 0, lib.BN_CALIB_SAVE, 1.0, None) == -1
    assert L.gs_bn_calib_fold(one, 1, one, 8, 3, 1.0, None) == -1
    assert L.gs_bn_calib_fold(one, 1, one, 8, -1, 1.0, None) == -1


class _FakeLoader:
    """Stands in for a training loader: records how it was requested, hands out CPU batches."""

    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw
        self.served = 0
        self.closed = False

    def __iter__(self):
        return self

    def __next__(self):
        self.served += 1
        return dict(img=torch.full((2, 3, 4, 4), float(self.served)), img_metas=[dict(), dict()],
                    gt_semantic_seg=torch.zeros(2, 1, 4, 4, dtype=torch.long))

    def close(self):
        self.closed = True


def _calib_cfg(**rc):
    return Config(dict(caliberate_bn=dict(recalibrate=dict(num_batches=3, **rc)),
                       data=dict(samples_per_gpu=2, workers_per_gpu=1,
                                 train=dict(type="SyntheticSegDataset", size=(8, 12)))))


def test_calibration_loader_is_rank_0_of_1_whatever_the_launch(monkeypatch):
    from gaia_seg_amd.core import dist as gdist
    monkeypatch.setattr(gdist, "rank", lambda: 3)
    monkeypatch.setattr(gdist, "world_size", lambda: 8)
    made = []

    def factory(*args, **kw):
        made.append(_FakeLoader(*args, **kw))
        return made[-1]
    batches = build_calibration_batches(_calib_cfg(seed=11), device="cpu", loader_factory=factory)
    (ld,) = made
    assert ld.kw["rank"] == 0 and ld.kw["world"] == 1 and ld.kw["seed"] == 11 and ld.kw["train"] is True
    assert ld.args[0]["type"] == "SyntheticSegDataset" and ld.args[1] == 2
    assert ld.served == 3 and ld.closed
    assert [float(b["img"][0, 0, 0, 0]) for b in batches] == [1.0, 2.0, 3.0]
    assert all(set(b) == {"img", "img_metas"} for b in batches)
    # the entry's own samples_per_gpu wins over data.samples_per_gpu
    build_calibration_batches(_calib_cfg(samples_per_gpu=4), device="cpu", loader_factory=factory)
    assert made[-1].args[1] == 4 and made[-1].kw["seed"] == 0
    # no key, no loader
    assert build_calibration_batches(Config(dict(data=dict(samples_per_gpu=2))), loader_factory=factory) is None
    assert len(made) == 2

    # through the real build_dataloader the override reaches the loader: rank 3 of 8 gets rank 0's batches
    from gaia_seg_amd.apis.train import build_dataloader
    got = build_calibration_batches(_calib_cfg(seed=5), device="cpu")
    own = iter(build_dataloader(dict(type="SyntheticSegDataset", size=(8, 12)), 2, seed=5, device="cpu"))
    zero = iter(build_dataloader(dict(type="SyntheticSegDataset", size=(8, 12)), 2, seed=5, device="cpu",
                                 rank=0, world=1))
    for b in got:
        assert torch.equal(b["img"], next(zero)["img"])
        assert not torch.equal(b["img"], next(own)["img"])


def test_model_space_loop_builds_its_calibrator_from_the_config_key():
    """tools/test_supernet.py hands test_model_space ``cfg.caliberate_bn`` and no calibrator: the key
    is parsed there, and the batches come from the config the model was built from."""
    import types
    from gaia_seg_amd.apis.test import test_model_space
    rows = [{"name": "a"}]
    with pytest.raises(ValueError, match="use_minibatch_stats"):
        test_model_space(types.SimpleNamespace(), [], rows, 1, 19,
                         calib_cfg=dict(recalibrate=dict(num_batches=2), use_minibatch_stats=True))
    with pytest.raises(ValueError, match="data.train"):      # a model built from a plain dict
        test_model_space(types.SimpleNamespace(top_cfg=None), [], rows, 1, 19,
                         calib_cfg=dict(recalibrate=dict(num_batches=2)))
