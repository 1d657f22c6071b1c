"""Elastic input resolution on one MI355X: gs_batch_rescale against
PyTorch-CPU F.interpolate, the runner / step graphs / ranking / finetune applying ``data.input_shape``
under ``apply_input_shape``, and the flag-off guard.

The training step is bit-reproducible run to run (tests/test_runner_gpu.py), so every comparison
between two runs here is exact equality."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from parity import train_step_parity
from util_models import ARCHS, arch_meta, fcn_head, make_batch, make_pair, model_cfg, psp_head, randomize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 64, 96
KEY = "data.input_shape"

# (h, w) -> (H, W): down, up, odd with a ragged store tail, aspect changed; then the degenerate ones
KERNEL_CASES = [((64, 96), (48, 72)), ((64, 96), (80, 120)), ((64, 96), (51, 77)), ((64, 96), (56, 100)),
                ((7, 5), (13, 3)), ((1, 9), (4, 9)), ((9, 1), (1, 1))]
IMG_TOL = 1e-5   # same fp32 weights as ATen's; the order of four fp32 roundings at |x| <~ 5 is ~1.5e-6


def _calls():
    from gaia_seg_amd.hip import ops
    return ops.BATCH_RESCALE_CALLS


def _rescale(img, gt, size):
    from gaia_seg_amd.hip import ops
    out, out_gt = ops.batch_rescale(img.cuda(), None if gt is None else gt.cuda(), size)
    torch.cuda.synchronize()
    return out.cpu(), None if out_gt is None else out_gt.cpu()


# ---- 1. the kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 1])
@pytest.mark.parametrize("src,dst", KERNEL_CASES)
def test_kernel_matches_cpu_interpolate(hip_lib, src, dst, n):
    """Image: bilinear, align_corners=False, fp32, max abs difference <= 1e-5 on N(0,1) data.  Labels:
    exactly ATen's nearest on the labels cast to float32 (exact for 0..255); 255 survives.  n = 1 makes
    the label count odd where H * W is (the one-label store tail)."""
    img, gt = make_batch(n, *src, seed=3)
    ref_img = F.interpolate(img, size=dst, mode="bilinear", align_corners=False)
    ref_gt = F.interpolate(gt.float(), size=dst, mode="nearest").long()
    out, out_gt = _rescale(img, gt, dst)
    assert out.shape == ref_img.shape and out.dtype == torch.float32
    assert out_gt.shape == ref_gt.shape and out_gt.dtype == torch.int64
    err = float((out - ref_img).abs().max())
    print("rescale %s -> %s n=%d: image max abs err %.3e" % (src, dst, n, err))
    assert torch.equal(out_gt, ref_gt)
    assert err <= IMG_TOL, err
    if src == (64, 96):
        assert int((out_gt == 255).sum()) > 0
    # a NULL label pointer: the image alone, the same values
    only, none = _rescale(img, None, dst)
    assert none is None and torch.equal(only, out)


def test_wrapper_passes_an_equal_size_through(hip_lib):
    img, gt = make_batch(N, H, W)
    img, gt = img.cuda(), gt.cuda()
    from gaia_seg_amd.hip import ops
    c0 = _calls()
    a, b = ops.batch_rescale(img, gt, (H, W))
    assert a is img and b is gt and _calls() == c0
    with pytest.raises(ValueError):
        ops.batch_rescale(img[:, :2], None, (8, 8))
    with pytest.raises(ValueError):
        ops.batch_rescale(img, gt[:, :, :-1], (8, 8))


# ---- helpers of the runner tests ----------------------------------------------------------------
def _anchor(name, scale=None):
    a = arch_meta(name)["backbone"]
    m = {"name": name, "arch.backbone.stem.width": a["stem"]["width"],
         "arch.backbone.body.width": a["body"]["width"], "arch.backbone.body.depth": a["body"]["depth"]}
    if scale is not None:
        m[KEY] = scale
    return m


def _metas(h=H, w=W):
    return [dict(ori_shape=(H, W, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False,
                 scale_factor=1.0) for _ in range(N)]


def _batch(seed, size=None, labels=True):
    """A 64x96 batch; ``size``: rescaled BEFOREHAND through ops' wrapper (labels too unless
    labels=False: evaluation keeps them at 64x96)."""
    from gaia_seg_amd.hip import ops
    img, gt = make_batch(N, H, W, seed=seed)
    img, gt = img.cuda(), gt.cuda()
    metas = _metas()
    if size is not None:
        img, g2 = ops.batch_rescale(img, gt if labels else None, size)
        gt = g2 if labels else gt
        metas = _metas(*size)
    return dict(img=img, img_metas=metas, gt_semantic_seg=gt)


def _model(seed=5, dropout=True):
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(copy.deepcopy(model_cfg(fcn_head(), aux=True)))
    randomize(model, seed)
    if not dropout:
        for h in (model.decode_head, model.auxiliary_head):
            h.dropout = None
    return model.cuda().train()


def _runner(model, **kw):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.05,
                             momentum=0.9, weight_decay=5e-4, max_iters=100, **kw)
    runner.register_hook(ArenaOptimizerHook())
    return runner, arena


def _train(steps, flag, **kw):
    """``steps``: [(anchor meta, batch)].  Returns the final state: parameters, momentum, buffers."""
    torch.manual_seed(0)
    model = _model(dropout=False)
    runner, arena = _runner(model, apply_input_shape=flag, **kw)
    seen = []
    for meta, batch in steps:
        runner.set_arch(meta)
        keep = (batch["img"], batch["gt_semantic_seg"], copy.deepcopy(batch["img_metas"]))
        runner.train_iter(batch)
        # the caller's batch is never modified
        assert batch["img"] is keep[0] and batch["gt_semantic_seg"] is keep[1] and batch["img_metas"] == keep[2]
        seen.append(runner.input_size)
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    state["__param"], state["__mom"] = arena.flat_param.clone(), arena.flat_mom.clone()
    return state, seen, runner


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ---- 2. the runner applies it, bitwise ------------------------------------------------------------
def test_runner_applies_input_shape_bitwise(hip_lib):
    scales = [48, 48, (56, 100)]
    sizes = [(48, 72), (48, 72), (56, 100)]
    c0 = _calls()
    flagged, seen, runner = _train([(_anchor("sub", s), _batch(i)) for i, s in enumerate(scales)], True)
    assert _calls() - c0 == 3 and seen == sizes
    plain, seen_p, _ = _train([(_anchor("sub"), _batch(i, size=sz)) for i, sz in enumerate(sizes)], False)
    assert seen_p == [None] * 3
    assert _same(flagged, plain)
    assert float(flagged["__mom"].abs().max()) > 0
    # and it is another training than the one at 64x96
    base, _, _ = _train([(_anchor("sub"), _batch(i)) for i in range(3)], False)
    assert not torch.equal(base["__param"], flagged["__param"])


def test_img_metas_follow_the_new_size(hip_lib):
    from gaia_seg_amd.core.input_shape import rescale_batch
    b = _batch(0)
    b["img_metas"][1].update(img_shape=(32, 96, 3), scale_factor=0.5)    # a crop inside its padding
    out, size = rescale_batch(b, (56, 100))
    assert size == (56, 100) and tuple(out["img"].shape) == (N, 3, 56, 100)
    assert tuple(out["gt_semantic_seg"].shape) == (N, 1, 56, 100)
    m0, m1 = out["img_metas"]
    assert m0["img_shape"] == (56, 100, 3) and m0["pad_shape"] == (56, 100, 3)
    assert m0["scale_factor"] == 56 / 64 and m0["ori_shape"] == (64, 96, 3) and m0["flip"] is False
    assert m1["img_shape"] == (28, 100, 3) and m1["pad_shape"] == (56, 100, 3)
    assert m1["scale_factor"] == 0.5 * 56 / 64
    assert b["img_metas"][0]["img_shape"] == (64, 96, 3) and b["img_metas"][0]["scale_factor"] == 1.0
    ev, _ = rescale_batch(b, 48, with_labels=False)
    assert tuple(ev["img"].shape) == (N, 3, 48, 72) and ev["gt_semantic_seg"] is b["gt_semantic_seg"]
    assert ev["img_metas"][0]["ori_shape"] == (64, 96, 3)
    same, size = rescale_batch(b, (3, 64, 96))
    assert same is b and size == (64, 96)


def test_bad_value_is_refused_at_first_sight(hip_lib):
    runner, _ = _runner(_model(), apply_input_shape=True)
    for bad in (0, (1, 48, 48), "48", 47.5):
        with pytest.raises(ValueError):
            runner.set_arch(_anchor("sub", bad))
    # a refused meta switches nothing: arch, name, key and scale stay those of the last good one
    runner.set_arch(_anchor("min", 48))
    depth = copy.deepcopy(runner.model.backbone.state_dict_of_arch())
    key = runner.arch_key
    with pytest.raises(ValueError):
        runner.set_arch(_anchor("sub", (1, 48, 48)))
    assert runner.model.backbone.state_dict_of_arch() == depth and runner.arch_key == key
    assert runner.arch_name == "min" and runner.input_shape == 48
    runner.set_arch(None)                    # "the current arch": no meta, so no scale either
    assert runner.input_shape is None
    off, _ = _runner(_model(), apply_input_shape=False)
    off.set_arch(_anchor("sub", 0))          # carried, not applied: nobody looks at it
    assert off.input_shape is None


# ---- 3. flag off ------------------------------------------------------------------------------------
def test_flag_off_is_the_training_without_the_key(hip_lib):
    scales = [48, (56, 100), 48]
    c0 = _calls()
    off, seen, _ = _train([(_anchor("sub", s), _batch(i)) for i, s in enumerate(scales)], False)
    assert _calls() == c0 and seen == [None] * 3
    bare, _, _ = _train([(_anchor("sub"), _batch(i)) for i in range(3)], False)
    assert _calls() == c0
    assert _same(off, bare)
    # flag on, target equal to the batch size (and a meta without the key): no launch, same training
    on, seen, _ = _train([(_anchor("sub", s), _batch(i))
                          for i, s in enumerate([64, (3, 64, 96), None])], True)
    assert _calls() == c0 and seen == [(64, 96)] * 3
    assert _same(on, bare)
    # flag on with another target: one launch per step
    _train([(_anchor("sub", 48), _batch(i)) for i in range(2)], True)
    assert _calls() == c0 + 2


# ---- 4. step graphs -----------------------------------------------------------------------------------
def test_step_graphs_one_per_subnet_and_resolution(hip_lib):
    """One anchor at two scales: two captured entries, and every replayed step bit-identical to the
    eager step (the pattern of test_step_graph_replay_equals_the_eager_step)."""
    from gaia_seg_amd.core.runner import PolyLrUpdaterHook

    def run(graphs):
        torch.manual_seed(0)
        model = _model(dropout=False)
        runner, arena = _runner(model, apply_input_shape=True)
        runner.graphs_enabled = graphs
        runner.register_hook(PolyLrUpdaterHook(power=0.9, min_lr=1e-4))
        runner.call_hook("before_run")
        logs = []
        for it, scale in enumerate([48, (56, 100), 48, (56, 100), 48, 48, (56, 100)]):
            runner.set_arch(_anchor("sub", scale))
            out = runner.train_iter(_batch(it))
            logs.append({k: float(v) for k, v in out["log_vars"].items()})
        torch.cuda.synchronize()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        shapes = sorted(tuple(e.static["img"].shape[-2:]) for e in runner._graphs.values())
        return sd, arena.flat_mom.detach().clone(), logs, dict(runner.graph_stats), shapes

    sd_e, mom_e, logs_e, st_e, _ = run(False)
    sd_g, mom_g, logs_g, st_g, shapes = run(True)
    assert st_e == {"captured": 0, "replayed": 0, "eager": 7}
    assert st_g == {"captured": 2, "replayed": 4, "eager": 1}, st_g
    assert shapes == [(48, 72), (56, 100)]
    assert logs_e == logs_g
    assert torch.equal(mom_e, mom_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


# ---- 5. parity at a rescaled size -------------------------------------------------------------------
@pytest.mark.parametrize("head", ["fcn", "psp"])
def test_train_step_parity_on_the_rescaled_batch(hip_lib, head):
    """The 51x77 batch the kernel produced through the whole model against the CPU oracle, at
    parity.py's own 1e-3 protocol (PSP's adaptive pooling bins are ragged at this size)."""
    cfg = model_cfg(fcn_head() if head == "fcn" else psp_head(), aux=True)
    prod, orc = make_pair(cfg)
    prod = prod.cuda().train()
    orc.train()
    meta = arch_meta("sub")
    prod.manipulate_arch(meta)
    orc.manipulate_arch(meta)
    img, gt = _rescale(*make_batch(N, H, W), (51, 77))
    assert tuple(img.shape) == (N, 3, 51, 77) and tuple(gt.shape) == (N, 1, 51, 77)
    train_step_parity(prod, orc, img, gt)


# ---- 6. ranking and finetune ------------------------------------------------------------------------
def _row(label, scale):
    a = ARCHS["sub"]
    return {"name": label, "arch.backbone.stem.width": a["stem"],
            "arch.backbone.body.width": tuple(a["width"]), "arch.backbone.body.depth": tuple(a["depth"]),
            KEY: scale, "overhead.flops": 1.0}


def test_model_space_ranking_at_each_rows_scale(hip_lib):
    from gaia_seg_amd.apis.test import test_model_space as rank
    from gaia_seg_amd.core.evaluation import evaluate_model
    model = _model().eval()
    loader = [_batch(11), _batch(12)]
    rows = [_row("s48", 48), _row("s64", 64)]
    c0 = _calls()
    on = rank(model, loader, rows, 2, 19, apply_input_shape=True)
    assert _calls() - c0 == 2                       # the 48 row's two batches; 64 passes through
    off = rank(model, loader, rows, 2, 19)
    assert _calls() - c0 == 2
    m = lambda r: tuple(r["metric.direct.%s" % k] for k in ("mIoU", "mAcc", "aAcc"))   # noqa: E731
    assert m(on[0]) != m(on[1])
    assert m(off[0]) == m(off[1]) == m(on[1])
    # without the argument the config the model was built from decides (tools/test_supernet.py)
    assert model.top_cfg is None
    model.top_cfg = dict(apply_input_shape=True)
    assert [m(r) for r in rank(model, loader, rows, 2, 19)] == [m(r) for r in on]
    assert [m(r) for r in rank(model, loader, rows, 2, 19, apply_input_shape=False)] == [m(r) for r in off]
    model.top_cfg = None
    assert on[0][KEY] == 48 and on[0]["overhead.flops"] == 1.0
    # each row equals evaluate_model on a loader rescaled beforehand (labels stay at 64x96)
    model.manipulate_arch(arch_meta("sub"))
    for row, size in zip(on, [(48, 72), None]):
        pre = [_batch(11, size, labels=False), _batch(12, size, labels=False)]
        assert tuple(pre[0]["gt_semantic_seg"].shape) == (N, 1, H, W)
        res = evaluate_model(model, pre, 2, 19)
        assert m(row) == (res["mIoU"], res["mAcc"], res["aAcc"])
    assert tuple(loader[0]["img"].shape) == (N, 3, H, W) and loader[0]["img_metas"] == _metas()


def test_finetune_at_the_rows_scale(hip_lib):
    """finetune_model_space with the flag: a row at scale 48 equals a fresh one-anchor run on batches
    rescaled beforehand; the supernet is restored afterwards."""
    from gaia_seg_amd.apis import set_random_seed
    from gaia_seg_amd.apis.finetune import finetune_model_space
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.evaluation import evaluate_model
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import ManipulateArchHook, PolyLrUpdaterHook

    def cfg(**kw):
        return Config(dict(optimizer=dict(type="SGD", lr=0.02, momentum=0.9, weight_decay=1e-4),
                           optimizer_config=dict(),
                           lr_config=dict(policy="poly", power=0.9, min_lr=1e-4, by_epoch=False),
                           runner=dict(type="IterBasedRunner", max_iters=3), data=dict(samples_per_gpu=N), **kw))

    def state(model):
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    model = _model()
    before = state(model)
    inside = {}
    rows = finetune_model_space(model, [_row("s48", 48)], cfg(apply_input_shape=True),
                                [_batch(s) for s in (3, 4, 5)], [_batch(11), _batch(12)], 2,
                                on_subnet=lambda row, m: inside.__setitem__(row["name"], state(m)))
    assert _same(state(model), before) and model.training           # the supernet is restored
    carried = finetune_model_space(_model(), [_row("s48", 48)], cfg(), [_batch(s) for s in (3, 4, 5)],
                                   [_batch(11), _batch(12)], 2)
    assert rows[0]["metric.finetune.mIoU"] != carried[0]["metric.finetune.mIoU"]

    fresh = _model()
    anchor = {"name": "s48", **{k: list(v) if isinstance(v, tuple) else v
                                for k, v in _row("s48", 48).items() if k != KEY}}
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(fresh)
    runner = IterBasedRunner(fresh, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.02,
                             momentum=0.9, weight_decay=1e-4, max_iters=3)
    runner.register_hook(ManipulateArchHook(build_model_sampler(dict(type="anchor", anchors=[anchor]))))
    runner.register_hook(PolyLrUpdaterHook(power=0.9, min_lr=1e-4, by_epoch=False))
    runner.register_hook(ArenaOptimizerHook())
    set_random_seed(0)
    runner.run([[_batch(s, (48, 72)) for s in (3, 4, 5)]])
    fresh.eval()
    fresh.manipulate_arch(arch_meta("sub"))
    res = evaluate_model(fresh, [_batch(s, (48, 72), labels=False) for s in (11, 12)], 2, 19)
    assert _same(state(fresh), inside["s48"])
    for k in ("mIoU", "mAcc", "aAcc"):
        assert res[k] == rows[0]["metric.finetune.%s" % k], k


def test_test_supernet_cli_ranks_rows_at_their_scale(tmp_path):
    """tools/test_supernet.py end to end on a tiny supernet: with the top-level apply_input_shape two
    rows of one arch at scales 48 and 64 get different metrics, without it equal ones."""
    import json
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    ck = os.path.join(str(tmp_path), "tiny.pth")
    save_checkpoint(_model(), ck, meta=dict(iter=0))
    space = os.path.join(str(tmp_path), "space.json")
    with open(space, "w") as fh:
        json.dump([{k: list(v) if isinstance(v, tuple) else v for k, v in r.items()}
                   for r in (_row("s48", 48), _row("s64", 64))], fh)
    cfg = dict(model=model_cfg(fcn_head(), aux=True), apply_input_shape=True,
               data=dict(samples_per_gpu=N, workers_per_gpu=0,
                         train=dict(type="SyntheticSegDataset", size=(H, W), num_classes=19)),
               evaluation=dict(num_batches=2))
    path = os.path.join(str(tmp_path), "rank_tiny.py")
    with open(path, "w") as fh:
        fh.write("".join("%s = %r\n" % kv for kv in cfg.items()))
    out = {}
    for tag, extra in (("on", []), ("off", ["--cfg-options", "apply_input_shape=False"])):
        wd = os.path.join(str(tmp_path), tag)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "test_supernet.py"), path, ck,
               "--model-space-path", space, "--work-dir", wd, "--seed", "0"] + extra
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        rows = json.load(open(os.path.join(wd, "test_supernet", "metrics.json")))
        out[tag] = {r["name"]: tuple(r["metric.direct.%s" % k] for k in ("mIoU", "mAcc", "aAcc")) for r in rows}
        assert [r[KEY] for r in rows] == [48, 64]
    assert out["on"]["s48"] != out["on"]["s64"]
    assert out["off"]["s48"] == out["off"]["s64"] == out["on"]["s64"]


def test_eval_hook_evaluates_val_anchors_at_their_scale(hip_lib):
    from gaia_seg_amd.core.evaluation import CrossArchEvalHook
    from gaia_seg_amd.core.model_space import build_model_sampler
    model = _model()
    runner, _ = _runner(model, apply_input_shape=True)
    runner.set_arch(_anchor("min", 48))
    a48, a64 = dict(_anchor("sub", 48), name="a48"), dict(_anchor("sub", 64), name="a64")
    sampler = build_model_sampler(dict(type="anchor", anchors=[a48, a64]))
    on = CrossArchEvalHook([_batch(5)], sampler, num_batches=1, apply_input_shape=True).evaluate(runner)
    off = CrossArchEvalHook([_batch(5)], sampler, num_batches=1).evaluate(runner)
    assert on["a48"]["mIoU"] != on["a64"]["mIoU"]
    assert off["a48"]["mIoU"] == off["a64"]["mIoU"] == on["a64"]["mIoU"]
    assert runner.input_shape == 48 and runner.arch_name == "min"     # the training draw survives


# ---- 7. CLI ---------------------------------------------------------------------------------------------
def test_train_supernet_cli_with_a_scale_sampler(tmp_path):
    """tools/train_supernet.py on the synthetic dataset, a 'candidate' scale sampler and the flag: the
    log shows more than one input size."""
    import re
    anchors = [_anchor("sub"), _anchor("min")]
    cfg = dict(
        model=model_cfg(fcn_head(), aux=True), apply_input_shape=True,
        train_sampler=dict(type="composite", model_samplers=[
            dict(type="candidate", key=KEY, candidates=(48, 56, 64, 80)),
            dict(type="anchor", anchors=anchors)]),
        val_sampler=dict(type="anchor", anchors=anchors),
        data=dict(samples_per_gpu=N, workers_per_gpu=0,
                  train=dict(type="SyntheticSegDataset", size=(H, W), num_classes=19)),
        optimizer=dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=0.0005), optimizer_config=dict(),
        lr_config=dict(policy="poly", power=0.9, min_lr=1e-4, by_epoch=False),
        runner=dict(type="IterBasedRunner", max_iters=8), log_config=dict(interval=1),
        checkpoint_config=dict(by_epoch=False, interval=100))
    path = os.path.join(str(tmp_path), "elastic_tiny.py")
    with open(path, "w") as fh:
        fh.write("".join("%s = %r\n" % kv for kv in cfg.items()))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_supernet.py"), path, "--work-dir",
           str(tmp_path), "--seed", "0", "--no-validate"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stderr + res.stdout
    sizes = set(re.findall(r"input: (\d+x\d+)", out))
    assert "Iter [8/8]" in out and "finished 8 iterations" in out
    assert len(sizes) > 1 and sizes <= {"48x72", "56x84", "64x96", "80x120"}, sizes
