"""The DynamicConvNeXtV2 backbone on the GPU against the float64 CPU model of tests/util_convnextv2.py carrying
the same weights: the tiny supernet (dims max (8, 16, 24, 32), depths max (2, 2, 3, 2)) on a 2x3x64x96 input, so
stage 4 is 2x3 pixels.  The GRN weights and biases and the LayerNorm affines are randomised to O(1): at the zero
init GRN is the identity, and a block that skipped it would pass every test.

Bounds: the four output features at conftest.rel_err <= 3e-5 (fp32 operators), every parameter gradient at the
1e-3 max norm of the baseline-config tests (tests/parity.py), gradient slices outside the active widths and
depths exactly zero."""
import copy
import os
import sys

import pytest
import torch

from conftest import rel_err
import util_convnextv2 as U
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FEAT_TOL = 3e-5
GRAD_TOL = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_backbone(seed=0):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg())
    U.randomize_convnextv2(m, seed)
    return m


_REF = {}


def reference(name):
    """(features, {parameter: gradient}) of subnet ``name`` in float64, computed once per session"""
    if name not in _REF:
        a = U.SUBNETS[name]
        m = make_backbone()
        sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
        img = make_batch(2, 64, 96, seed=1)[0]
        outs = U.convnextv2_ref(sd, img.double(), a["width"], a["depth"])
        cots = cotangents(outs)
        sum((o * c.double()).sum() for o, c in zip(outs, cots)).backward()
        _REF[name] = ([o.detach() for o in outs], {k: v.grad for k, v in sd.items()})
    return _REF[name]


def cotangents(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(o.shape, generator=g) for o in outs]


@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name):
    a = U.SUBNETS[name]
    feats_r, grads_r = reference(name)
    m = make_backbone().to(DEV).train()
    m.manipulate_arch({"body": {"width": a["width"], "depth": a["depth"]}})
    img = make_batch(2, 64, 96, seed=1)[0].to(DEV)
    outs = m(img)
    assert [tuple(o.shape) for o in outs] == [(2, w, 16 >> i, 24 >> i) for i, w in enumerate(a["width"])]
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        err = rel_err(o, r)
        print("%s: feature %d rel_err %.3g" % (name, i, err))
        assert err <= FEAT_TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    worst = {}
    for k, p in m.named_parameters():
        ref, got = grads_r[k], p.grad
        if got is not None and ref is not None and ref.dim() == 2:
            got = got[:, :, 0, 0]                                # a linear weight: [out, in] in the state dict
        if ref is None or float(ref.abs().max()) == 0:          # a block the depth skips
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert got is not None, k
        worst[k] = rel_err(got, ref)
        assert bool((got.cpu()[ref == 0] == 0).all()), "%s: gradient outside the active slice" % k
    w = max(worst, key=worst.get)
    print("%s: %d parameter gradients, worst %s %.3g" % (name, len(worst), w, worst[w]))
    assert any(k.endswith("grn.weight") for k in worst) and any(k.endswith("grn.bias") for k in worst)
    assert worst[w] <= GRAD_TOL, {k: v for k, v in worst.items() if v > GRAD_TOL}
    if name == "sub":    # the slices beyond the active widths, and the skipped blocks
        assert float(m.stem.weight.grad[4:].abs().max()) == 0
        blk = m.stage(1)[0]                                      # width 8 of 16
        assert float(blk.pwconv1.weight.grad[32:].abs().max()) == 0
        assert float(blk.pwconv1.weight.grad[:, 8:].abs().max()) == 0
        assert float(blk.grn.weight.grad[..., :32].abs().max()) > 0 and float(blk.grn.bias.grad[..., :32].abs().max()) > 0
        assert float(blk.grn.weight.grad[..., 32:].abs().max()) == 0 and float(blk.grn.bias.grad[..., 32:].abs().max()) == 0
        g = m.stage(0)[1].grn.weight.grad
        assert g is None or float(g.abs().max()) == 0


def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(U.tiny_model_cfg()))
    U.randomize_convnextv2(model.backbone, seed)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _batch(seed):
    img, gt = make_batch(2, 64, 96, seed=seed)
    metas = [dict(ori_shape=(64, 96, 3), img_shape=(64, 96, 3), flip=False) for _ in range(2)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def test_adamw_training_iterations_touch_the_active_ranges_only(hip_lib):
    """three AdamW iterations (sub, sub, max) under the recipe of the supernet config: no decay on norms and GRN"""
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    model = _model()
    optimizer = dict(type="AdamW", lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05,
                     paramwise_cfg=dict(norm_decay_mult=0., custom_keys={"grn": dict(decay_mult=0.)}))
    opt = check_optimizer_cfg(optimizer)
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=100,
                             param_groups=build_param_groups(model, optimizer))
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    for it in range(2):
        runner.set_arch(U.arch_meta("sub"))
        out = runner.train_iter(_batch(it))
        torch.cuda.synchronize()
        assert all(v == v and abs(v) < 1e6 for v in (float(x) for x in out["log_vars"].values()))
    after = dict(model.named_parameters())
    changed = lambda k: not torch.equal(after[k], before[k])      # noqa: E731
    s = "backbone.encoder.stages."
    assert changed("backbone.embeddings.patch_embeddings.weight") and changed(s + "0.layers.0.grn.weight")
    assert changed(s + "2.layers.1.pwconv2.weight") and changed(s + "2.downsampling_layer.0.weight")
    assert changed(s + "1.layers.1.grn.bias") and changed("decode_head.conv_seg.weight")
    for k in before:          # blocks beyond the sampled depths (1, 2, 2, 1) took no part
        if any(k.startswith(s + "%d.layers.%d." % (i, j)) for i, j in ((0, 1), (2, 2), (3, 1))):
            assert not changed(k), k
    # GRN beyond the active 4w channels: no gradient and no decay, so bit for bit what it was
    for k, n in ((s + "0.layers.0.grn.weight", 16), (s + "1.layers.1.grn.bias", 32)):
        assert torch.equal(after[k][..., n:], before[k][..., n:]), k
        assert not torch.equal(after[k][..., :n], before[k][..., :n]), k
    # a conv weight beyond its active slice only decays
    w0, w1 = before["backbone.embeddings.patch_embeddings.weight"], after["backbone.embeddings.patch_embeddings.weight"]
    assert float((w1[4:] - w0[4:] * (1 - 1e-3 * 0.05) ** 2).abs().max()) < 1e-6
    mid = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner.set_arch(U.arch_meta("max"))
    out = runner.train_iter(_batch(2))
    torch.cuda.synchronize()
    assert all(v == v for v in (float(x) for x in out["log_vars"].values()))
    after = dict(model.named_parameters())
    assert not torch.equal(after[s + "3.layers.1.grn.weight"], mid[s + "3.layers.1.grn.weight"])
    assert model.backbone.stage(3).depth_state == 2


def test_step_graph_replay_equals_the_eager_step(hip_lib):
    """tests/test_runner_gpu.py's criterion on the ConvNeXt V2 model: parameters, momentum and logged losses of
    replayed step graphs are bit-identical to eager steps."""
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner

    def run(graphs):
        model = _model()
        arena = ParamArena(model)
        runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.05,
                                 momentum=0.9, weight_decay=1e-4, max_iters=100)
        runner.register_hook(ArenaOptimizerHook())
        runner.graphs_enabled = graphs
        runner.call_hook("before_run")
        logs = []
        for it, name in enumerate(["sub", "max", "sub", "max", "sub"]):
            runner.set_arch(U.arch_meta(name))
            out = runner.train_iter(_batch(it))
            logs.append({k: float(v) for k, v in out["log_vars"].items()})
        torch.cuda.synchronize()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return sd, arena.flat_mom.detach().clone(), logs, dict(runner.graph_stats)

    sd_e, mom_e, logs_e, st_e = run(False)
    sd_g, mom_g, logs_g, st_g = run(True)
    assert st_e == {"captured": 0, "replayed": 0, "eager": 5}
    assert st_g["captured"] >= 1 and st_g["replayed"] >= 1, st_g
    assert logs_e == logs_g
    assert all(v == v for log in logs_e for v in log.values())
    assert torch.equal(mom_e, mom_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


def test_extracted_subnet_equals_the_supernet_slice_bit_for_bit(hip_lib):
    from extract_subnet import extract
    sup = _model().eval()
    n_sup = sum(p.numel() for p in sup.parameters())
    meta = U.arch_meta("sub")
    a = U.SUBNETS["sub"]
    img = make_batch(2, 64, 96, seed=3)[0].to(DEV)
    sup.manipulate_arch({"backbone": {"body": {"width": a["width"], "depth": a["depth"]}}})
    with torch.no_grad():
        want = [f.clone() for f in sup.backbone(img)]
        want_logits = sup.encode_decode(img, None).clone()
    sup.deploy()
    sub = extract(sup, meta)
    sup.deploy(False)
    assert sum(p.numel() for p in sup.parameters()) == n_sup          # supernet untouched
    bb = sub.backbone
    assert [len(bb.stage(i)) for i in range(4)] == a["depth"]
    blk = bb.stage(1)[0]
    assert tuple(blk.dwconv.weight.shape) == (8, 1, 7, 7) and tuple(blk.grn.weight.shape) == (1, 1, 1, 32)
    assert tuple(blk.grn.bias.shape) == (1, 1, 1, 32) and blk.grn.dim == 32
    assert tuple(blk.pwconv1.weight.shape) == (32, 8, 1, 1) and tuple(blk.layernorm.weight.shape) == (8,)
    assert tuple(bb.state_dict()["encoder.stages.1.layers.0.pwconv2.weight"].shape) == (8, 32)
    assert tuple(bb.stem.weight.shape) == (4, 3, 4, 4) and tuple(bb.out_norm(3).weight.shape) == (16,)
    assert U.convnextv2_param_count(a["width"], a["depth"]) == sum(p.numel() for p in bb.parameters())
    with torch.no_grad():
        got = sub.backbone(img)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert torch.equal(sub.encode_decode(img, None), want_logits)
