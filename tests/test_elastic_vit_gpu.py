"""The ElasticTransformer backbone and DynamicMultiLevelNeck on the GPU against the float64 CPU model of
tests/util_vit.py carrying the same weights: a tiny supernet (embed_dim max 128, 2 heads max, num_layers
[1, 2, 1], img_size (32, 48), patch 16, so N = 7 tokens) and its subnets 'max' and 'sub' (D = 64, heads
[1, 2, 1], layers [1, 1, 1], ratios [30, 40, 35]).

Bounds: features and every active parameter's gradient at the 1e-3 max norm of the baseline-config tests
(tests/parity.py); gradients of inactive slices, skipped layers, the relative-position tables and the final
ln1 exactly zero or absent."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_vit as U
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = U.TINY["img_size"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_backbone(seed=0):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg())
    U.randomize_vit(m, seed)
    return m


def cotangents(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(o.shape, generator=g) for o in outs]


_REF = {}


def reference(name):
    """(features, {parameter: gradient}) of subnet ``name`` in float64, computed once per session"""
    if name not in _REF:
        m = make_backbone()
        sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
        img = make_batch(2, H, W, seed=1)[0]
        outs = U.vit_ref(sd, img.double(), U.SUBNETS[name])
        sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
        _REF[name] = ([o.detach() for o in outs], {k: v.grad for k, v in sd.items()})
    return _REF[name]


@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name):
    a = U.SUBNETS[name]
    feats_r, grads_r = reference(name)
    m = make_backbone().to(DEV).train()
    m.manipulate_arch(U.arch_of(name))
    img = make_batch(2, H, W, seed=1)[0].to(DEV)
    outs = m(img)
    assert [tuple(o.shape) for o in outs] == [(2, a["embed_dim"], H // 16, W // 16)] * 4
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        err = rel_err(o, r)
        print("%s: feature %d rel_err %.3g" % (name, i, err))
        assert err <= TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    worst = {}
    for k, p in m.named_parameters():
        ref, got = grads_r[k], p.grad
        if got is not None and ref is not None and ref.dim() == 2:
            got = got[:, :, 0, 0]                                # a linear weight: [out, in] in the state dict
        idx = U.active_slice(k, a, 7)
        if idx is None:          # a skipped layer, the relative-position tables, the final ln1
            assert ref is None or float(ref.abs().max()) == 0
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert got is not None, k
        outside = torch.ones(ref.shape, dtype=torch.bool)
        outside[idx] = False
        assert not bool(ref[outside].any())
        assert not bool(got.cpu()[outside].any()), "%s: gradient outside the active slice" % k
        if k.endswith("attn.w_ks.bias"):
            # softmax does not see a shift common to all keys' scores, so this gradient is exactly 0 in
            # exact arithmetic and rounding noise in any floating one (float64 included): there is no
            # relative error to take.  It is a sum of dS * Q like the query bias's is of dS * K, so the
            # bound is absolute, TOL of that sibling's largest element.
            bound = TOL * float(grads_r[k.replace("w_ks", "w_qs")].abs().max())
            assert float(ref.abs().max()) <= bound and float(got.abs().max()) <= bound, k
            continue
        worst[k] = rel_err(got, ref)
    w = max(worst, key=worst.get)
    print("%s: %d parameter gradients, worst %s %.3g" % (name, len(worst), w, worst[w]))
    assert worst[w] <= TOL, {k: v for k, v in worst.items() if v > TOL}
    assert "cls_token" in worst and "pos_embed" in worst and "elastic_encoder3.0.attn.w_ks.weight" in worst
    assert len(worst) == 4 + sum(a["layers"]) * 15
    if name == "sub":    # the slices beyond the active widths, and the skipped layer
        assert float(m.cls_token.grad[..., 64:].abs().max()) == 0
        assert float(m.elastic_encoder1[0].attn.w_qs.weight.grad[64:].abs().max()) == 0
        assert float(m.elastic_encoder1[0].attn.proj.weight.grad[:, 64:].abs().max()) == 0
        assert float(m.elastic_encoder1[0].mlp.layer1.weight.grad[192:].abs().max()) == 0
        g = m.elastic_encoder2[1].mlp.layer1.weight.grad
        assert g is None or float(g.abs().max()) == 0


def test_an_input_of_another_size_is_refused(hip_lib):
    m = make_backbone().to(DEV)
    with pytest.raises(ValueError, match="img_size"):
        m(torch.zeros(1, 3, 32, 32, device=DEV))


def test_neck_against_float64_with_a_downsampling_level(hip_lib):
    """default scales [0.5, 1, 2, 4] on 4 x 6 maps; the active input width (24 of 32) comes with the map"""
    from gaia_seg_amd.models import build_neck
    torch.manual_seed(4)
    neck = build_neck(dict(type="DynamicMultiLevelNeck", in_channels=[32] * 4, out_channels=16,
                           conv_cfg=dict(type="DynConv2d")))
    with torch.no_grad():
        for p in neck.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.2)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in neck.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    xs = [torch.randn(2, 24, 4, 6, generator=g) for _ in range(4)]
    want = []
    for i, x in enumerate(xs):
        y = F.conv2d(x.double(), sd["lateral_convs.%d.conv.weight" % i][:, :24], sd["lateral_convs.%d.conv.bias" % i])
        y = F.interpolate(y, scale_factor=neck.scales[i], mode="bilinear", align_corners=False)
        want.append(F.conv2d(y, sd["convs.%d.conv.weight" % i], sd["convs.%d.conv.bias" % i], padding=1))
    cots = cotangents(want)
    sum((o * c.double()).sum() for o, c in zip(want, cots)).backward()
    neck = neck.to(DEV).train()
    ins = [x.to(DEV).requires_grad_(True) for x in xs]
    outs = neck(tuple(ins))
    assert [tuple(o.shape[2:]) for o in outs] == [(2, 3), (4, 6), (8, 12), (16, 24)]
    for o, r in zip(outs, want):
        assert rel_err(o, r) <= 3e-5
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cots])
    for k, p in neck.named_parameters():
        assert rel_err(p.grad, sd[k].grad) <= TOL, k
        if k.startswith("lateral_convs") and k.endswith("weight"):
            assert float(p.grad[:, 24:].abs().max()) == 0


def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(U.tiny_model_cfg()))
    U.randomize_vit(model.backbone, seed)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _runner(model, lr=0.05):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=lr,
                             momentum=0.9, weight_decay=1e-4, max_iters=100)
    runner.register_hook(ArenaOptimizerHook())
    return runner, arena


def _batch(seed):
    img, gt = make_batch(2, H, W, seed=seed)
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), flip=False) for _ in range(2)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def _one_step():
    model = _model()
    runner, _ = _runner(model)
    runner.call_hook("before_run")
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner.set_arch(U.arch_meta("sub"))
    out = runner.train_iter(_batch(0))
    torch.cuda.synchronize()
    return model, before, {k: float(v) for k, v in out["log_vars"].items()}


def test_one_runner_step_moves_the_active_parameters_only_and_repeats_bit_for_bit(hip_lib):
    model, before, logs = _one_step()
    assert logs and all(v == v and abs(v) < 1e6 for v in logs.values()), logs
    after = dict(model.named_parameters())
    active = {id(p) for p in model.active_parameters()}
    n_active = n_idle = 0
    for k, p in after.items():
        moved = not torch.equal(p, before[k])
        if id(p) in active:
            assert moved, "%s is active and did not change" % k
            n_active += 1
        else:
            assert not moved, "%s is inactive and changed" % k
            n_idle += 1
    idle = [k for k, p in after.items() if id(p) not in active]
    assert any(k.startswith("backbone.elastic_encoder2.1.") for k in idle)
    assert any("rel_pos_embed" in k for k in idle) and "backbone.ln1.weight" in idle
    assert n_active > 60 and n_idle >= 16 + 16 + 2
    # beyond the active slice a used tensor only decays (no gradient)
    w0, w1 = before["backbone.cls_token"], after["backbone.cls_token"]
    assert float((w1[..., 64:] - w0[..., 64:] * (1 - 0.05 * 1e-4)).abs().max()) < 1e-7
    # the same step from the same snapshot
    model2, before2, logs2 = _one_step()
    assert logs2 == logs
    for k, p in model2.named_parameters():
        assert torch.equal(before2[k], before[k]), k
        assert torch.equal(p, after[k]), "%s differs between two identical steps" % k


def test_extracted_subnet_equals_the_supernet_slice_bit_for_bit(hip_lib):
    from extract_subnet import extract
    sup = _model().eval()
    n_sup = sum(p.numel() for p in sup.parameters())
    a = U.SUBNETS["sub"]
    img = make_batch(2, H, W, seed=3)[0].to(DEV)
    sup.manipulate_arch({"backbone": U.arch_of("sub")})
    with torch.no_grad():
        want = [f.clone() for f in sup.backbone(img)]
        want_logits = sup.encode_decode(img, None).clone()
    sup.deploy()
    sub = extract(sup, U.arch_meta("sub"))
    sup.deploy(False)
    assert sum(p.numel() for p in sup.parameters()) == n_sup          # supernet untouched
    bb = sub.backbone
    assert [len(getattr(bb, n)) for n in bb.layers] == a["layers"]
    layer = bb.elastic_encoder1[0]
    sd = bb.state_dict()
    assert tuple(sd["elastic_encoder1.0.attn.w_qs.weight"].shape) == (64, 64)
    assert tuple(sd["elastic_encoder2.0.attn.proj.weight"].shape) == (64, 128)
    assert tuple(sd["elastic_encoder3.0.mlp.layer1.weight"].shape) == (224, 64)
    assert tuple(sd["elastic_encoder3.0.mlp.layer2.weight"].shape) == (64, 224)
    assert tuple(layer.norm1.weight.shape) == (64,) and tuple(bb.cls_token.shape) == (1, 1, 64)
    assert tuple(bb.pos_embed.shape) == (1, 7, 64) and tuple(bb.norm1.weight.shape) == (64,)
    assert tuple(bb.elastic_patch_embed.projection.weight.shape) == (64, 3, 16, 16)
    assert tuple(sub.neck.lateral_convs[0].conv.weight.shape) == (16, 64, 1, 1)
    # the deployed subnet's checkpoint loads back into a model of its size, strictly
    twin = copy.deepcopy(sub)
    with torch.no_grad():
        for p in twin.parameters():
            p.zero_()
    twin.load_state_dict(sub.state_dict(), strict=True)
    with torch.no_grad():
        got = sub.backbone(img)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert torch.equal(sub.encode_decode(img, None), want_logits)
        assert torch.equal(twin.encode_decode(img, None), want_logits)


def test_slide_evaluation_with_the_crop_equal_to_img_size(hip_lib):
    """test_cfg.mode='slide' with crop_size = stride = img_size on an image of 2 x 2 windows: the class
    probabilities are those of the four windows, each evaluated on its own (fp32 evaluations of the same
    resize + softmax: the bound is the fp32 operator bound, probabilities being O(1))"""
    from gaia_seg_amd.core.config import ConfigDict
    model = _model().eval()
    model.test_cfg = ConfigDict(mode="slide", crop_size=(H, W), stride=(H, W))
    img = make_batch(2, 2 * H, 2 * W, seed=5)[0].to(DEV)
    metas = [dict(ori_shape=(2 * H, 2 * W, 3), img_shape=(2 * H, 2 * W, 3), flip=False) for _ in range(2)]
    with torch.no_grad():
        probs = model.inference(img, metas, rescale=False)
        assert tuple(probs.shape) == (2, 19, 2 * H, 2 * W)
        for y0 in (0, H):
            for x0 in (0, W):
                want = model.encode_decode(img[:, :, y0:y0 + H, x0:x0 + W].contiguous(), None).softmax(dim=1)
                assert rel_err(probs[:, :, y0:y0 + H, x0:x0 + W], want) <= 3e-5, (y0, x0)
        labels = model.simple_test_device(img, metas, rescale=True)
    assert tuple(labels.shape) == (2, 2 * H, 2 * W) and labels.dtype == torch.int64
