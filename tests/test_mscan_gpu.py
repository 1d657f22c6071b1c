"""DynamicMSCAN and the segmentor it makes with the UPer head, on the GPU against the float64 CPU restatement
of tests/util_mscan.py carrying the same weights.  The tiny supernet: widths 16/24/32/40, depths 2/1/2/1,
ratios 4/4/2/2; subnet 'sub': widths 8/16/24/32, depths 1/1/1/1, ratios 2/4/2/1.  On 2 x 3 x 64 x 96 images
the stage maps are 16x24, 8x12, 4x6 and 2x3, so almost every strip of the 1x21 / 21x1 pairs hangs over a
border.

Bounds: features and every active parameter's gradient at the 1e-3 max norm of the end-to-end tests of the
other backbones (tests/parity.py); gradients of inactive slices and skipped blocks exactly zero or absent.
A BatchNorm-adjacent parameter (BN_ADJACENT) whose gradient misses 1e-3 is held to the conditioning rule of
tests/parity.py instead: the same network in fp32 on the CPU is measured against float64, the HIP error may
be at most COND_FACTOR times that (the stage-4 BatchNorms normalise 12 values per channel), and the ratio
joins parity.POOLED_RATIOS.  No other parameter may miss 1e-3.  (Measured on an MI355X: no parameter needed
the rule; the worst gradient of 'max' is 1.8e-6 from float64, of 'sub' 2.9e-6.)"""
import copy
import os
import sys

import pytest
import torch

from conftest import rel_err
from parity import COND_FACTOR, POOLED_RATIOS
import util_mscan as U
from util_models import make_batch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = 64, 96
# the BatchNorms' own parameters, and the patch-embedding convs, each of which feeds one
BN_ADJACENT = ("patch_embed", ".norm1.", ".norm2.")


def make_backbone(seed=0):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg())
    U.randomize_mscan(m, seed)
    return m


def cotangents(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(o.shape, generator=g) for o in outs]


_REF = {}


def reference(name, dtype=torch.float64):
    """(features, {parameter: gradient}) of subnet ``name`` in ``dtype`` on the CPU, computed once per session"""
    if (name, dtype) not in _REF:
        m = make_backbone()
        sd = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v)
              for k, v in m.state_dict().items()}
        img = make_batch(2, H, W, seed=1)[0]
        outs = U.mscan_ref(sd, img.to(dtype), U.SUBNETS[name])
        sum((o * c.to(dtype)).sum() for o, c in zip(outs, cotangents(outs))).backward()
        _REF[(name, dtype)] = ([o.detach() for o in outs],
                               {k: v.grad for k, v in sd.items() if v.is_floating_point()})
    return _REF[(name, dtype)]


@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name):
    a = U.SUBNETS[name]
    feats_r, grads_r = reference(name)
    m = make_backbone().to(DEV).train()
    m.manipulate_arch(U.arch_of(name))
    img = make_batch(2, H, W, seed=1)[0].to(DEV)
    outs = m(img)
    assert [tuple(o.shape) for o in outs] == [(2, c, H >> s, W >> s) for c, s in zip(a["width"], (2, 3, 4, 5))]
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        err = rel_err(o, r)
        print("%s: feature %d rel_err %.3g" % (name, i, err))
        assert err <= TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    worst, conditioned, null = {}, {}, []
    for k, p in m.named_parameters():
        ref, got = grads_r[k], p.grad
        idx = U.active_slice(k, a)
        if idx is None:          # a block past the stage's depth
            assert ref is None or float(ref.abs().max()) == 0
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert got is not None, k
        outside = torch.ones(ref.shape, dtype=torch.bool)
        outside[idx] = False
        assert not bool(ref[outside].any())
        assert not bool(got.cpu()[outside].any()), "%s: gradient outside the active slice" % k
        if k.startswith("patch_embed") and k.endswith(("proj.bias", "proj.0.bias", "proj.3.bias")):
            # a BatchNorm on batch statistics does not see a shift of its input: exactly 0 in exact
            # arithmetic and rounding noise in any floating one, so the bound is absolute, TOL of the same
            # conv's largest weight gradient (as for k_proj.bias in tests/test_mit_gpu.py)
            bound = TOL * float(grads_r[k[:-4] + "weight"].abs().max())
            assert float(ref.abs().max()) <= bound and float(got.abs().max()) <= bound, k
            null.append(k)
            continue
        err = rel_err(got, ref)
        if err > TOL:            # the rule of tests/parity.py: a bounded factor of fp32's own error
            # ... open to a BatchNorm's own parameters and to the conv that feeds one, to nothing else
            assert any(t in k for t in BN_ADJACENT), "%s: %.3g" % (k, err)
            own = rel_err(reference(name, torch.float32)[1][k], ref)
            conditioned[k] = (err, own)
            assert err <= COND_FACTOR * own, "%s: %.3g against fp32's own %.3g" % (k, err, own)
            POOLED_RATIOS.append(err / own)
        else:
            worst[k] = err
    w = max(worst, key=worst.get)
    print("%s: %d parameter gradients within %g, worst %s %.3g; conditioned: %s"
          % (name, len(worst), TOL, w, worst[w], conditioned))
    assert len(null) == 5 and len(worst) + len(conditioned) + len(null) == 8 + 3 * 4 + 4 * 2 + sum(a["depth"]) * 32
    if name == "sub":    # the slices beyond the active widths, and the skipped blocks
        sgu = m.block2[0].attn.spatial_gating_unit
        assert float(m.patch_embed2.proj.weight.grad[16:].abs().max()) == 0
        assert float(m.patch_embed3.proj.weight.grad[:, 16:].abs().max()) == 0
        assert float(sgu.conv2_1.weight.grad[16:].abs().max()) == 0 and float(sgu.conv0.bias.grad[16:].abs().max()) == 0
        assert float(m.block1[0].mlp.fc1.weight.grad[16:].abs().max()) == 0
        assert float(m.block1[0].layer_scale_1.grad[8:].abs().max()) == 0
        g = m.block1[1].attn.spatial_gating_unit.conv0.weight.grad
        assert g is None or float(g.abs().max()) == 0


def test_eval_mode_uses_the_running_statistics(hip_lib):
    m = make_backbone().to(DEV).eval()
    m.manipulate_arch(U.arch_of("sub"))
    img = make_batch(2, H, W, seed=2)[0]
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v for k, v in m.state_dict().items()}
    want = U.mscan_ref(sd, img.double(), U.SUBNETS["sub"], training=False)
    with torch.no_grad():
        got = m(img.to(DEV))
    for i, (g, r) in enumerate(zip(got, want)):
        assert rel_err(g, r) <= TOL, i


# ---- the segmentor -----------------------------------------------------------------------------------------
def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    from util_models import randomize
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(U.tiny_model_cfg()))
    randomize(model.decode_head, seed + 1)
    randomize(model.auxiliary_head, seed + 2)
    U.randomize_mscan(model.backbone, seed)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _runner(model):
    """AdamW as the recipe configures it, without the schedule (its warm-up scales the first steps to
    nothing)"""
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", (0.9, 0.999), 1e-8)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=6e-5, momentum=0.0,
                             weight_decay=0.01, max_iters=100)
    runner.register_hook(ArenaOptimizerHook())
    return runner


def _batch(seed, h=H, w=W, n=2):
    img, gt = make_batch(n, h, w, seed=seed)
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False) for _ in range(n)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def _one_step(monkeypatch):
    monkeypatch.delenv("GS_STEP_GRAPH", raising=False)
    model = _model()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner = _runner(model)
    runner.call_hook("before_run")
    runner.set_arch(U.arch_meta("sub"))
    out = runner.train_iter(_batch(0))
    torch.cuda.synchronize()
    return model, before, {k: float(v) for k, v in out["log_vars"].items()}


def test_one_adamw_step_of_the_tiny_segmentor_twice(hip_lib, monkeypatch):
    model, before, log = _one_step(monkeypatch)
    print(log)
    assert log and all(v == v and abs(v) < 1e6 for v in log.values()), log
    assert {"decode.loss_seg", "aux.loss_seg", "loss"} <= set(log)
    after = dict(model.named_parameters())
    sgu = "backbone.block1.0.attn.spatial_gating_unit."
    for k in (sgu + "conv0.weight", sgu + "conv2_1.weight", sgu + "conv2_2.bias", sgu + "conv3.weight",
              "backbone.block1.0.layer_scale_1", "backbone.patch_embed1.proj.0.weight", "decode_head.conv_seg.weight"):
        assert not torch.equal(after[k], before[k]), "%s did not move" % k
    skipped = "backbone.block1.1.attn.spatial_gating_unit.conv0.weight"
    assert torch.equal(after[skipped], before[skipped]), "a skipped block's parameter moved"
    model2, _, log2 = _one_step(monkeypatch)
    assert log2 == log
    for (k, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), "%s: two identical runs differ" % k


def test_whole_image_inference(hip_lib):
    model = _model().eval()
    img = make_batch(1, H, W, seed=5)[0].to(DEV)
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), flip=False)]
    with torch.no_grad():
        whole = model.inference(img, metas, rescale=False)
        assert tuple(whole.shape) == (1, 19, H, W) and bool(torch.isfinite(whole).all())
        assert rel_err(whole, model.encode_decode(img, None).softmax(dim=1)) <= 3e-5
        labels = model.simple_test_device(img, metas, rescale=True)
    assert tuple(labels.shape) == (1, H, W) and labels.dtype == torch.int64


def test_extracted_subnet_equals_the_supernet_slice_bit_for_bit(hip_lib):
    from extract_subnet import extract
    sup = _model().eval()
    n_sup = sum(p.numel() for p in sup.parameters())
    a = U.SUBNETS["sub"]
    img = make_batch(2, H, W, seed=3)[0].to(DEV)
    sup.manipulate_arch({"backbone": U.arch_of("sub")})
    with torch.no_grad():
        want = [f.clone() for f in sup.backbone(img)]
    sup.deploy()
    sub = extract(sup, U.arch_meta("sub"))
    sup.deploy(False)
    assert sum(p.numel() for p in sup.parameters()) == n_sup          # supernet untouched
    bb = sub.backbone
    assert [len(bb.stage(i)[1]) for i in range(4)] == a["depth"]
    plain = U.PlainMSCAN(a).state_dict()
    got = bb.state_dict()
    assert list(got) == list(plain)
    for k, v in plain.items():
        assert tuple(got[k].shape) == tuple(v.shape), k
    assert U.param_count(a) == sum(p.numel() for p in bb.parameters())
    with torch.no_grad():
        for g, w in zip(sub.backbone(img), want):
            assert torch.equal(g, w)
