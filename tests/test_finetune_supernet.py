"""Fast-finetune without a GPU: the command line of tools/finetune_supernet.py, the anchor sampler
built from a meta, the --resume filter and row merge, the set-up refusals of
apis.finetune.finetune_model_space, and the loaders' restart."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location(
        "finetune_supernet_tool", os.path.join(ROOT, "tools", "finetune_supernet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R50 = {"name": "R50", "arch.backbone.stem.width": 32, "arch.backbone.body.width": (48, 96, 192, 384),
       "arch.backbone.body.depth": (3, 4, 6, 3), "data.input_shape": (512, 2048),
       "overhead.flops": 2.385e11, "metric.direct.mIoU": 0.41, "metric.direct.mAcc": 0.5,
       "metric.direct.aAcc": 0.9}
R77 = dict(R50, name="R77", **{"arch.backbone.body.depth": (3, 4, 15, 3), "metric.direct.mIoU": 0.44})
ANON = {k: v for k, v in dict(R50, **{"arch.backbone.body.depth": (4, 6, 29, 4)}).items() if k != "name"}


# ---- command line ------------------------------------------------------------------------------
def test_parse_args_accepts_the_reference_flags(tool, monkeypatch):
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    a = tool.parse_args(["cfg.py"])
    assert (a.config, a.work_dir, a.no_validate, a.load_from, a.model_space_path) == ("cfg.py", None, False, None, None)
    assert (a.metric_tag, a.out_name, a.seed, a.deterministic, a.launcher) == ("finetune", "metrics.json", None, False, "none")
    assert a.eval == ["mIoU"] and not a.resume and not a.keep_checkpoints
    assert os.environ["LOCAL_RANK"] == "0"
    a = tool.parse_args(["cfg.py", "--work-dir", "w", "--no-validate", "--load-from", "ck.pth",
                         "--model-space-path", "ms.json", "--metric-tag", "ft2", "--out-name", "o.json",
                         "--seed", "3", "--deterministic", "--cfg-options", "runner.max_iters=2", "a.b=1",
                         "--launcher", "pytorch", "--local_rank", "1", "--eval", "mIoU", "--gpus", "1",
                         "--tmpdir", "/tmp/x", "--gpu-collect", "--resume", "--keep-checkpoints"])
    assert (a.work_dir, a.no_validate, a.load_from, a.model_space_path) == ("w", True, "ck.pth", "ms.json")
    assert (a.metric_tag, a.out_name, a.seed, a.deterministic, a.launcher) == ("ft2", "o.json", 3, True, "pytorch")
    assert a.cfg_options == ["runner.max_iters=2", "a.b=1"] and a.local_rank == 1
    assert a.resume and a.keep_checkpoints and a.gpus == 1 and a.gpu_collect and a.tmpdir == "/tmp/x"
    assert tool.parse_args(["cfg.py", "--gpu-ids", "0", "1"]).gpu_ids == [0, 1]
    assert tool.parse_args(["cfg.py", "--options", "a=1"]).options == ["a=1"]


@pytest.mark.parametrize("extra, words", [
    (["--save-results"], "--save-results"),
    (["--out", "res.pkl"], "--out"),
    (["--eval-options", "a=1"], "--eval-options"),
    (["--launcher", "slurm"], "--launcher slurm is not supported"),
    (["--launcher", "mpi"], "--launcher mpi is not supported"),
    (["--eval", "mDice"], "only mIoU"),
    (["--options", "a=1", "--cfg-options", "b=2"], "cannot be both"),
    (["--gpus", "1", "--gpu-ids", "0"], "not allowed with"),
])
def test_parse_args_refuses_loudly(tool, capsys, extra, words):
    with pytest.raises(SystemExit) as e:
        tool.parse_args(["cfg.py"] + extra)
    assert e.value.code == 2
    assert words in capsys.readouterr().err


def test_main_requires_checkpoint_and_model_space(tool, tmp_path):
    cfg = os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_finetune.py")
    with pytest.raises(SystemExit, match="checkpoint is required"):
        tool.main([cfg, "--work-dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="not existed"):
        tool.main([cfg, "--work-dir", str(tmp_path), "--load-from", str(tmp_path / "none.pth")])
    ck = tmp_path / "ck.pth"
    ck.write_bytes(b"")
    with pytest.raises(SystemExit, match="model space is required"):
        tool.main([cfg, "--work-dir", str(tmp_path), "--load-from", str(ck)])


def test_example_config(tool, tmp_path):
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_finetune.py"))
    assert cfg.model.decode_head.type == "DynamicFCNHead"
    assert "model_space_path" in cfg and "load_from" in cfg
    assert cfg.lr_config.policy == "poly" and cfg.lr_config.by_epoch is False
    assert cfg.runner.max_iters <= 1000
    rule = dict(cfg.model_sampling_rules)
    assert (rule["type"], rule["operation"], rule["key"]) == ("sample", "top", "metric.direct.mIoU")
    rows = [dict(R50, name="n%d" % i, **{"arch.backbone.body.depth": (3, 4, 6 + i, 3),
                                          "metric.direct.mIoU": 0.01 * ((7 * i) % 12)}) for i in range(12)]
    path = tmp_path / "ms.json"
    path.write_text(json.dumps([{k: list(v) if isinstance(v, tuple) else v for k, v in r.items()}
                                for r in rows]))
    got = tool.select_metas(cfg, str(path))
    want = sorted(rows, key=lambda r: r["metric.direct.mIoU"], reverse=True)[:rule["value"]]
    assert [r["name"] for r in got] == [r["name"] for r in want]


# ---- anchor sampler, rows, resume --------------------------------------------------------------
def test_anchor_sampler_cfg_has_the_reference_form():
    """tools/finetune_supernet.py:283-288: {'type': 'anchor', 'anchors': [{'name': str(i), **meta}]}."""
    from gaia_seg_amd.apis.finetune import anchor_sampler_cfg
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.model_space import arch_key, build_model_sampler
    c = anchor_sampler_cfg(ANON, 7)
    assert set(c) == {"type", "anchors"} and c["type"] == "anchor" and len(c["anchors"]) == 1
    a = c["anchors"][0]
    assert a["name"] == "7"                                   # the row index, as a string
    assert a["arch.backbone.body.depth"] == [4, 6, 29, 4]     # lists: the form manipulate_arch takes
    assert {k: v for k, v in a.items() if k != "name"}.keys() == ANON.keys()
    assert arch_key(a) == arch_key(ANON)
    assert anchor_sampler_cfg(R50, 7)["anchors"][0]["name"] == "R50"   # **meta wins over str(i)
    assert "name" not in ANON and isinstance(R50["arch.backbone.body.depth"], tuple)   # inputs untouched
    s = build_model_sampler(anchor_sampler_cfg(R77, 0))
    assert [s.sample()["name"] for _ in range(3)] == ["R77"] * 3 and len(s.traverse()) == 1
    assert fold_dict(s.sample())["arch"]["backbone"]["body"]["depth"] == [3, 4, 15, 3]


def test_row_keeps_the_columns_of_other_tags():
    from gaia_seg_amd.apis.finetune import finetune_row
    res = dict(mIoU=0.5, mAcc=0.6, aAcc=0.7, IoU=[0.5], Acc=[0.6])
    row = finetune_row(R50, res, "finetune")
    assert {k: row[k] for k in R50} == R50
    assert set(row) - set(R50) == {"metric.finetune.mIoU", "metric.finetune.mAcc", "metric.finetune.aAcc"}
    assert (row["metric.finetune.mIoU"], row["metric.finetune.mAcc"], row["metric.finetune.aAcc"]) == (0.5, 0.6, 0.7)
    assert "metric.finetune.mIoU" not in R50
    again = finetune_row(row, dict(res, mIoU=0.9), "ft2")      # a second tag on top of the first
    assert again["metric.finetune.mIoU"] == 0.5 and again["metric.ft2.mIoU"] == 0.9
    assert again["metric.direct.mIoU"] == 0.41


def test_resume_filter_and_merge(tool, tmp_path):
    from gaia_seg_amd.apis.finetune import finetune_row
    from gaia_seg_amd.core.model_space import load_model_space
    metas = [R77, R50, ANON]
    res = dict(mIoU=0.5, mAcc=0.6, aAcc=0.7)
    done50 = finetune_row(R50, res, "finetune")
    other_tag = finetune_row(R77, res, "ft2")                  # another tag does not count
    partial = dict(ANON, **{"metric.finetune.mIoU": 0.1})      # a torn row does not count either
    assert tool.pending_metas(metas, [], "finetune") == metas
    assert tool.pending_metas(metas, [done50, other_tag, partial], "finetune") == [R77, ANON]
    assert tool.pending_metas(metas, [done50, other_tag], "ft2") == [R50, ANON]
    # matching is by arch, not by name or by the other columns
    renamed = dict(done50, name="other", **{"overhead.flops": 1.0})
    assert tool.pending_metas(metas, [renamed], "finetune") == [R77, ANON]
    # the file round trip (lists in the file, tuples in memory) keeps the filter exact
    out = tmp_path / "m.json"
    tool.write_rows([done50], str(out))
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    existing = load_model_space(str(out))
    assert tool.pending_metas(metas, existing, "finetune") == [R77, ANON]
    # merge: selection order, fresh rows and kept rows, then the existing rows outside the selection
    new77 = finetune_row(R77, dict(res, mIoU=0.8), "finetune")
    outside = finetune_row(dict(R50, name="X", **{"arch.backbone.body.depth": (1, 1, 1, 1)}), res, "finetune")
    merged = tool.merge_rows(metas, existing + [outside], [new77], "finetune")
    assert [r.get("name") for r in merged] == ["R77", "R50", "X"]
    assert merged[0]["metric.finetune.mIoU"] == 0.8 and merged[1] == existing[0]
    assert tool.checkpoint_name(R50) == "R50" and tool.checkpoint_name(dict(R50, name="a/b c")) == "a_b_c"
    assert len(tool.checkpoint_name(ANON)) == 8 and tool.checkpoint_name(ANON) == tool.checkpoint_name(dict(ANON))


# ---- refusals at set-up ------------------------------------------------------------------------
class _Refuse:
    """Stands in for the model: any touch means the set-up went past the check."""

    def __getattr__(self, name):
        raise AssertionError("set-up touched the model (%s) before refusing" % name)


def _cfg(**kw):
    from gaia_seg_amd.core.config import Config
    base = dict(optimizer=dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=0.0),
                optimizer_config=dict(), lr_config=dict(policy="poly", power=0.9, min_lr=1e-4, by_epoch=False),
                runner=dict(type="IterBasedRunner", max_iters=3), data=dict(samples_per_gpu=2))
    base.update(kw)
    return Config(base)


def test_refusals_before_the_model_is_touched(monkeypatch):
    import torch
    from gaia_seg_amd.apis import finetune_model_space
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(ValueError, match="use_distillation"):
        finetune_model_space(_Refuse(), [R50], _cfg(use_distillation=True), [], [], 1)
    with pytest.raises(ValueError, match="use_minibatch_stats"):
        finetune_model_space(_Refuse(), [R50], _cfg(caliberate_bn=dict(use_minibatch_stats=True)), [], [], 1)
    for empty in ([], None, ()):
        with pytest.raises(ValueError, match="no subnet"):
            finetune_model_space(_Refuse(), empty, _cfg(), [], [], 1)
    # what training refuses anyway is refused here too, before the snapshot is taken
    with pytest.raises(NotImplementedError, match="lr_config.policy"):
        finetune_model_space(_Refuse(), [R50], _cfg(lr_config=dict(policy="step", step=[2])), [], [], 1)
    with pytest.raises(NotImplementedError, match="dynamic loss scaling"):
        finetune_model_space(_Refuse(), [R50], _cfg(optimizer_config=dict(type="Fp16OptimizerHook",
                                                                         loss_scale="dynamic")), [], [], 1)
    with pytest.raises(NotImplementedError, match="grad_clip"):
        finetune_model_space(_Refuse(), [R50], _cfg(optimizer_config=dict(grad_clip=dict(max_norm=1))), [], [], 1)
    # reset_stats alone is honoured, not refused: it gets past the checks and reaches the model
    with pytest.raises(AssertionError, match="touched the model"):
        finetune_model_space(_Refuse(), [R50], _cfg(caliberate_bn=dict(reset_stats=True)), [], [], 1)


def test_train_segmentor_still_refuses_fp16_with_distillation_first():
    """train_segmentor became a thin caller of prepare_training + run_training: its own refusal still
    comes before the model is moved."""
    from gaia_seg_amd.apis.train import train_segmentor
    cfg = _cfg(use_distillation=True, optimizer_config=dict(type="Fp16OptimizerHook", loss_scale=512.))
    with pytest.raises(ValueError, match="use_distillation"):
        train_segmentor(_Refuse(), None, None, None, cfg)


# ---- the train data restarts -------------------------------------------------------------------
def test_synthetic_loader_restart():
    import torch
    from gaia_seg_amd.core.synthetic import SyntheticLoader
    ld = SyntheticLoader(1, (8, 8), seed=3, device="cpu", pool=3)
    first = [next(ld)["img"].clone() for _ in range(4)]
    ld.restart()
    again = [next(ld)["img"] for _ in range(4)]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], first[1])


class _DrawingPipeline:
    """Stands in for GpuTrainPipeline (which needs the GPU): one augmentation draw per batch."""

    def __init__(self, seed=None, **kw):
        import numpy as np
        self.rng = np.random.RandomState(seed)

    def batch(self, samples):
        return [s[2] for s in samples], float(self.rng.rand())


def test_file_loader_restart_replays_the_stream_and_keeps_decoding_work(tmp_path, monkeypatch):
    import gaia_seg_amd.datasets.loader as loader_mod
    from gaia_seg_amd.datasets import build_dataset, train_pipeline_kwargs
    from test_datasets import TRAIN_PIPELINE, make_cityscapes
    make_cityscapes(str(tmp_path), cities=(("a", 4), ("b", 3)))
    ds = build_dataset(dict(type="CityscapesDataset", data_root=str(tmp_path), img_dir="leftImg8bit/train",
                            ann_dir="gtFine/train", pipeline=TRAIN_PIPELINE))
    monkeypatch.setattr(loader_mod, "GpuTrainPipeline", _DrawingPipeline)
    ld = loader_mod.FileBatchLoader(ds, 2, train_pipeline_kwargs(ds.pipeline), workers_per_gpu=2, seed=5,
                                    device="cpu")
    first = [next(ld) for _ in range(5)]          # into the second epoch (3 batches per epoch)
    assert ld.epoch >= 1
    ld.restart()
    assert ld.epoch == 0 and not ld._pre.pending
    again = [next(ld) for _ in range(5)]
    ld.close()
    assert again == first                          # same files in the same order, same draws
    fresh = loader_mod.FileBatchLoader(ds, 2, train_pipeline_kwargs(ds.pipeline), seed=5, device="cpu")
    assert [next(fresh) for _ in range(5)] == first
    fresh.close()
