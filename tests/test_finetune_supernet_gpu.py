"""Fast-finetune on one MI355X: apis.finetune.finetune_model_space in process on the tiny supernet
(FCN head plus auxiliary head, 64x96, bs 2, 3 iterations, subnets 'sub' and 'min'), and
tools/finetune_supernet.py end to end behind the other three tools of the workflow.

The training step is bit-reproducible run to run (tests/test_runner_gpu.py compares separate runs
bitwise), so every comparison between two runs here is exact equality."""
import copy
import importlib.util
import json
import math
import os
import subprocess
import sys
import types

import pytest
import torch

from util_models import ARCHS, arch_meta, fcn_head, make_batch, model_cfg, randomize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 64, 96
MAX_ITERS = 3


def _meta(label, arch):
    a = ARCHS[arch]
    return {"name": label, "arch.backbone.stem.width": a["stem"],
            "arch.backbone.body.width": tuple(a["width"]), "arch.backbone.body.depth": tuple(a["depth"]),
            "overhead.flops": float(sum(a["width"])), "metric.direct.mIoU": 0.25}


A, B = _meta("A", "sub"), _meta("B", "min")


def _batches(seeds):
    out = []
    for s in seeds:
        img, gt = make_batch(N, H, W, seed=s)
        metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False)
                 for _ in range(N)]
        out.append(dict(img=img.cuda(), img_metas=metas, gt_semantic_seg=gt.cuda()))
    return out


def _cfg(lr=0.02, weight_decay=1e-4, min_lr=1e-4, **kw):
    from gaia_seg_amd.core.config import Config
    base = dict(optimizer=dict(type="SGD", lr=lr, momentum=0.9, weight_decay=weight_decay),
                optimizer_config=dict(),
                lr_config=dict(policy="poly", power=0.9, min_lr=min_lr, by_epoch=False),
                runner=dict(type="IterBasedRunner", max_iters=MAX_ITERS), data=dict(samples_per_gpu=N))
    base.update(kw)
    return Config(base)


def _model(seed=5):
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(copy.deepcopy(model_cfg(fcn_head(), aux=True)))
    randomize(model, seed)
    return model.cuda().train()


def _state(model):
    """{name: CPU copy} of every parameter and buffer (state_dict folds the pending batch counts in)."""
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


class _Run:
    """One finetune_model_space call on a fresh tiny supernet: rows, the state before and after, the
    state inside on_subnet per name, and the arena the call built."""

    def __init__(self, metas, cfg=None, model=None, **kw):
        from gaia_seg_amd.apis import finetune as ft
        self.model = model if model is not None else _model()
        self.model.manipulate_arch(arch_meta("min"))      # some arch that is neither A's nor the max
        self.arch_before = copy.deepcopy(self.model.backbone.state_dict_of_arch())
        self.before = _state(self.model)
        self.inside = {}
        made = []
        real = ft.prepare_training
        ft.prepare_training = lambda m, c: made.append(real(m, c)) or made[-1]
        try:
            self.rows = ft.finetune_model_space(
                self.model, metas, cfg or _cfg(), _batches((3, 4, 5)), _batches((11, 12)), 2,
                on_subnet=lambda row, m: self.inside.__setitem__(row["name"], _state(m)), **kw)
        finally:
            ft.prepare_training = real
        self.arena = made[0][1]
        self.after = _state(self.model)
        self.arch_after = copy.deepcopy(self.model.backbone.state_dict_of_arch())
        self.by_name = {r["name"]: r for r in self.rows}


@pytest.fixture(scope="module")
def run_ab():
    return _Run([A, B])


@pytest.fixture(scope="module")
def active_slices():
    """{parameter / buffer name: shape of its leading active slice} of subnet A, from the project's
    own pruning (tools/extract_subnet.py): a name that is missing belongs to a depth-skipped block."""
    spec = importlib.util.spec_from_file_location("extract_subnet_tool",
                                                  os.path.join(ROOT, "tools", "extract_subnet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from gaia_seg_amd.models import build_segmentor
    cfg = tool.prepare_cfg(types.SimpleNamespace(model=copy.deepcopy(model_cfg(fcn_head(), aux=True))))
    model = build_segmentor(cfg.model).cuda().eval()
    model.deploy()
    sub = tool.extract(model, {k: list(v) if isinstance(v, tuple) else v for k, v in A.items()})
    return {k: tuple(v.shape) for k, v in sub.state_dict().items()}


def _split(name, tensor, slices):
    """(active leading slice, mask of the elements outside it) of a supernet tensor."""
    mask = torch.ones(tensor.shape, dtype=torch.bool)
    shape = slices.get(name)
    if shape is None:
        return None, mask
    idx = tuple(slice(0, s) for s in shape)
    mask[idx] = False
    return idx, mask


# ---- 1. restoration ---------------------------------------------------------------------------
def test_supernet_is_restored(run_ab, hip_lib):
    r = run_ab
    assert [x["name"] for x in r.rows] == ["A", "B"]
    assert _same(r.before, r.after)                               # parameters AND buffers, bit for bit
    assert not _same(r.before, r.inside["A"]) and not _same(r.before, r.inside["B"])
    a = r.arena
    assert float(a.flat_mom.abs().max()) == 0.0 and float(a.flat_grad.abs().max()) == 0.0
    assert a.flat_acc is None or float(a.flat_acc.abs().max()) == 0.0
    assert a.grads_clean
    assert r.arch_after == r.arch_before and r.arch_before["body"]["depth"] == [1, 1, 1, 1]
    assert r.model.training
    assert [m.fp16_enabled for m in r.model.modules() if hasattr(m, "fp16_enabled")].count(True) == 0
    assert hip_lib.gs_get_train_precision() == 0
    for m in r.model.modules():
        assert not getattr(m, "_nbt_pending", 0)
    for row in r.rows:
        assert row["metric.direct.mIoU"] == 0.25 and row["overhead.flops"] > 0    # other columns kept
        for k in ("mIoU", "mAcc", "aAcc"):
            assert math.isfinite(row["metric.finetune.%s" % k]) and 0.0 <= row["metric.finetune.%s" % k] <= 1.0


def test_eval_mode_model_comes_back_in_eval_mode():
    m = _model().eval()
    r = _Run([B], model=m)
    assert not r.model.training and _same(r.before, r.after)


# ---- 2. order invariance ----------------------------------------------------------------------
def test_rows_do_not_depend_on_order_or_company(run_ab):
    ba, only_a = _Run([B, A]), _Run([A])
    assert [x["name"] for x in ba.rows] == ["B", "A"]
    for other in (ba, only_a):
        for name, row in other.by_name.items():
            assert row == run_ab.by_name[name], name               # exact float equality
            assert _same(other.inside[name], run_ab.inside[name]), name


# ---- 3. same as the long way ------------------------------------------------------------------
def test_equals_a_fresh_anchor_run_of_the_existing_pieces(run_ab):
    """The yardstick is the code that was there before: a fresh model with the same weights, an
    IterBasedRunner with ManipulateArchHook over the one-anchor sampler, the same lr and optimizer
    hooks, the same batches and seed, then evaluate_model."""
    from gaia_seg_amd.apis import set_random_seed
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.evaluation import evaluate_model
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, IterBasedRunner, ManipulateArchHook,
                                          PolyLrUpdaterHook)
    model = _model()
    anchor = {"name": "A", **{k: list(v) if isinstance(v, tuple) else v for k, v in A.items()}}
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.02,
                             momentum=0.9, weight_decay=1e-4, max_iters=MAX_ITERS)
    runner.register_hook(ManipulateArchHook(build_model_sampler(dict(type="anchor", anchors=[anchor]))))
    runner.register_hook(PolyLrUpdaterHook(power=0.9, min_lr=1e-4, by_epoch=False))
    runner.register_hook(ArenaOptimizerHook())
    set_random_seed(0)
    runner.run([_batches((3, 4, 5))])
    assert runner.iter == MAX_ITERS
    model.eval()
    model.manipulate_arch(fold_dict(anchor)["arch"])
    res = evaluate_model(model, _batches((11, 12)), 2, 19)
    assert _same(_state(model), run_ab.inside["A"])
    for k in ("mIoU", "mAcc", "aAcc"):
        assert res[k] == run_ab.by_name["A"]["metric.finetune.%s" % k], k


# ---- 4. it trains, and only where it should ----------------------------------------------------
def test_trains_the_active_slices_only(run_ab, active_slices):
    """Without weight decay every element outside A's active slices -- depth-skipped blocks and the
    trailing width slices of used tensors -- is bitwise S0 inside on_subnet, and every active
    trainable tensor has moved.  With weight decay (run_ab) the depth-skipped blocks are still
    bitwise S0; the trailing slices of USED tensors decay, as documented in core/param_arena.py
    (torch.optim.SGD decays the whole tensor of a parameter that has a gradient), so for them the
    statement holds at weight_decay=0 only."""
    r = _Run([A], cfg=_cfg(weight_decay=0.0))
    params = dict(r.model.named_parameters())
    assert any(k not in active_slices for k in params)             # A skips blocks
    moved_outside, unmoved_active, narrowed = [], [], 0
    for name in params:
        s0, ft = r.before[name], r.inside["A"][name]
        idx, outside = _split(name, s0, active_slices)
        narrowed += int(idx is not None and bool(outside.any()))
        if not torch.equal(s0[outside], ft[outside]):
            moved_outside.append(name)
        if idx is not None and params[name].requires_grad and torch.equal(s0[idx], ft[idx]):
            unmoved_active.append(name)
    assert narrowed > 10                                           # A narrows tensors as well
    assert not moved_outside, moved_outside[:5]
    assert not unmoved_active, unmoved_active[:5]
    skipped = [k for k in run_ab.before if k not in active_slices]
    assert skipped and all(torch.equal(run_ab.before[k], run_ab.inside["A"][k]) for k in skipped)


# ---- 5. zero learning rate: calibration only ---------------------------------------------------
def test_zero_lr_recalibrates_batchnorm_only(active_slices):
    from gaia_seg_amd.apis.test import test_model_space as direct_rows
    model = _model()
    direct = direct_rows(model.eval(), _batches((11, 12)), [A], 2, 19)[0]
    model.train()
    r = _Run([A], cfg=_cfg(lr=0.0, min_lr=0.0), model=model)
    s0, ft = r.before, r.inside["A"]
    for name, _ in r.model.named_parameters():
        assert torch.equal(s0[name], ft[name]), name
    stats = [k for k in s0 if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(stats) > 20
    for name in stats:
        idx, outside = _split(name, s0[name], active_slices)
        assert torch.equal(s0[name][outside], ft[name][outside]), name
        if idx is not None:
            assert not torch.equal(s0[name][idx], ft[name][idx]), name
    for name in (k for k in s0 if k.endswith("num_batches_tracked")):
        steps = MAX_ITERS if name in active_slices else 0
        assert int(ft[name]) == int(s0[name]) + steps, name
    got = tuple(r.rows[0]["metric.finetune.%s" % k] for k in ("mIoU", "mAcc", "aAcc"))
    assert got != tuple(direct["metric.direct.%s" % k] for k in ("mIoU", "mAcc", "aAcc"))
    assert _same(r.before, r.after)


def test_reset_stats_is_honoured(active_slices):
    """caliberate_bn.reset_stats: every turn starts from running_mean 0 / running_var 1, so after
    3 steps of momentum 0.1 an inactive slice reads exactly 0 / 1, and S0 still comes back."""
    r = _Run([A], cfg=_cfg(lr=0.0, min_lr=0.0, caliberate_bn=dict(reset_stats=True)))
    ft = r.inside["A"]
    for name in (k for k in ft if k.endswith("running_var")):
        _, outside = _split(name, ft[name], active_slices)
        assert bool((ft[name][outside] == 1).all()), name
        assert bool((ft[name.replace("running_var", "running_mean")][outside] == 0).all()), name
    assert _same(r.before, r.after)


# ---- 6. fp16 ----------------------------------------------------------------------------------
def test_fp16_hook_runs_and_leaves_no_trace(hip_lib, run_ab):
    seen = []
    cfg = _cfg(optimizer_config=dict(type="Fp16OptimizerHook", loss_scale=512.))
    model = _model()
    from gaia_seg_amd.apis import finetune_model_space
    before = _state(model)
    rows = finetune_model_space(model, [A, B], cfg, _batches((3, 4, 5)), _batches((11, 12)), 2,
                                on_subnet=lambda row, m: seen.append((m.fp16_enabled, _state(m))))
    assert [s[0] for s in seen] == [True, True]                    # evaluated in fp16, as mmcv's hook
    for row in rows:
        for k in ("mIoU", "mAcc", "aAcc"):
            assert math.isfinite(row["metric.finetune.%s" % k]) and 0.0 <= row["metric.finetune.%s" % k] <= 1.0
    assert hip_lib.gs_get_train_precision() == 0 and hip_lib.gs_get_forward_precision() == 0
    assert [m.fp16_enabled for m in model.modules() if hasattr(m, "fp16_enabled")].count(True) == 0
    assert _same(before, _state(model))
    assert not _same(seen[0][1], run_ab.inside["A"])               # fp16 operands did take part


# ---- 7. one checkpoint read for the whole model space -------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("finetune_supernet_tool",
                                                  os.path.join(ROOT, "tools", "finetune_supernet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_checkpoint_is_read_once(tmp_path, monkeypatch):
    """tools/finetune_supernet.py main() in process on the tiny supernet (two subnets selected out
    of three): every checkpoint read goes through torch.load, which is counted."""
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    src = build_segmentor(copy.deepcopy(model_cfg(fcn_head(), aux=True)))
    randomize(src, 5)
    ck = str(tmp_path / "supernet.pth")
    save_checkpoint(src, ck, meta=dict(iter=7))
    cfg_path = tmp_path / "tiny_finetune.py"
    cfg_path.write_text(
        "model = %r\n"
        "data = dict(samples_per_gpu=%d, workers_per_gpu=2,\n"
        "            train=dict(type='SyntheticSegDataset', size=(%d, %d), num_classes=19))\n"
        "optimizer = dict(type='SGD', lr=0.02, momentum=0.9, weight_decay=1e-4)\n"
        "optimizer_config = dict()\n"
        "lr_config = dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False)\n"
        "runner = dict(type='IterBasedRunner', max_iters=%d)\n"
        "evaluation = dict(interval=100, metric='mIoU', num_batches=2)\n"
        "log_config = dict(interval=1)\n"
        "model_sampling_rules = dict(type='sample', operation='top', key='metric.direct.mIoU', value=2)\n"
        % (model_cfg(fcn_head(), aux=True), N, H, W, MAX_ITERS))
    space = tmp_path / "space.json"
    rows_in = [dict(A, **{"metric.direct.mIoU": 0.2}), dict(B, **{"metric.direct.mIoU": 0.3}),
               dict(_meta("C", "max"), **{"metric.direct.mIoU": 0.1})]
    space.write_text(json.dumps([{k: list(v) if isinstance(v, tuple) else v for k, v in r.items()}
                                 for r in rows_in]))
    reads = []
    real_load = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: reads.append(a[0]) or real_load(*a, **k))
    _tool().main([str(cfg_path), "--load-from", ck, "--model-space-path", str(space),
                  "--work-dir", str(tmp_path / "w"), "--seed", "0", "--no-validate"])
    assert reads == [ck]
    rows = json.load(open(tmp_path / "w" / "finetune_supernet" / "metrics.json"))
    assert [r["name"] for r in rows] == ["B", "A"]                 # the rule's order: best direct mIoU first
    assert all(math.isfinite(r["metric.finetune.mIoU"]) and r["metric.direct.mIoU"] in (0.2, 0.3) for r in rows)


# ---- the command line, behind the other three tools ---------------------------------------------
def _run(cmd, timeout):
    res = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res


def test_finetune_supernet_cli_end_to_end(tmp_path):
    from gaia_seg_amd.core.checkpoint import load_checkpoint
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.model_space import ModelSpace
    from gaia_seg_amd.models import build_segmentor
    cfgs = os.path.join(ROOT, "configs", "supernet")
    tr = tmp_path / "train"
    _run([os.path.join(ROOT, "tools", "train_supernet.py"), os.path.join(cfgs, "fcn_ar50to101v2.py"),
          "--work-dir", str(tr), "--seed", "0", "--no-validate", "--max-iters", "2", "--cfg-options",
          "data.train.size=(128,256)", "log_config.interval=1", "checkpoint_config.interval=2"], 600)
    ck = str(tr / "iter_2.pth")
    test_cfg = os.path.join(cfgs, "fcn_ar50to101v2_test_supernet.py")
    space = str(tmp_path / "flops.json")
    _run([os.path.join(ROOT, "tools", "count_flops.py"), test_cfg, "--out", space], 300)
    wd = tmp_path / "work"
    small = ["data.train.size=(128,256)", "evaluation.num_batches=2"]
    _run([os.path.join(ROOT, "tools", "test_supernet.py"), test_cfg, ck, "--model-space-path", space,
          "--work-dir", str(wd), "--seed", "0", "--cfg-options", "data.samples_per_gpu=1"] + small, 600)
    direct = json.load(open(wd / "test_supernet" / "metrics.json"))
    assert sorted(r["name"] for r in direct) == ["R101", "R50", "R77"]
    top2 = sorted(direct, key=lambda r: r["metric.direct.mIoU"], reverse=True)[:2]

    tool = os.path.join(ROOT, "tools", "finetune_supernet.py")
    cfg_path = os.path.join(cfgs, "fcn_ar50to101v2_finetune.py")
    cmd = [tool, cfg_path, "--load-from", ck, "--model-space-path", str(wd / "test_supernet" / "metrics.json"),
           "--work-dir", str(wd), "--seed", "0", "--keep-checkpoints", "--cfg-options",
           "model_sampling_rules.value=2", "runner.max_iters=2", "log_config.interval=1"] + small
    res = _run(cmd, 600)
    log = res.stdout + res.stderr
    assert log.count("Iter [2/2]") == 2, log[-2000:]
    out = wd / "finetune_supernet" / "metrics.json"
    rows = json.load(open(out))
    assert [r["name"] for r in rows] == [r["name"] for r in top2]
    by_direct = {r["name"]: r for r in direct}
    for r in rows:
        for k in ("mIoU", "mAcc", "aAcc"):
            assert r["metric.direct.%s" % k] == by_direct[r["name"]]["metric.direct.%s" % k]
            v = r["metric.finetune.%s" % k]
            assert math.isfinite(v) and 0.0 <= v <= 1.0
        assert r["overhead.flops"] == by_direct[r["name"]]["overhead.flops"]
    best = ModelSpace.load(str(out)).apply_rule(
        dict(type="sample", operation="top", key="metric.finetune.mIoU", value=1)).rows
    assert len(best) == 1 and best[0]["metric.finetune.mIoU"] == max(r["metric.finetune.mIoU"] for r in rows)

    # --resume: everything is done already -- same rows, no training iteration
    res = _run(cmd[:2] + ["--resume"] + cmd[2:], 600)
    log = res.stdout + res.stderr
    assert "Iter [" not in log and "nothing left to finetune" in log, log[-2000:]
    assert json.load(open(out)) == rows

    # a kept checkpoint is a supernet checkpoint with the row as its meta
    cfg = Config.fromfile(cfg_path)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    kept = load_checkpoint(model, str(wd / "finetune_supernet" / "ckpt" / ("%s.pth" % rows[0]["name"])), strict=True)
    assert kept["meta"]["name"] == rows[0]["name"]
    assert kept["meta"]["metric.finetune.mIoU"] == rows[0]["metric.finetune.mIoU"]
    assert kept["meta"]["arch.backbone.body.depth"] == rows[0]["arch.backbone.body.depth"]
    sup = torch.load(ck, map_location="cpu")["state_dict"]
    assert any(not torch.equal(sup[k], v) for k, v in model.state_dict().items() if k in sup)
