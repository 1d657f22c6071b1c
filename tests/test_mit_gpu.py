"""DynamicMixVisionTransformer, DynamicSegformerHead and the segmentor they make, on the GPU against float64
CPU restatements carrying the same weights: tests/util_mit.py for the backbone (which tests/test_mit.py ties
to transformers' SegformerModel), this file for the head and the losses.  The tiny supernet: heads 1/2/3/2
(widths 64/128/192/128), depths 1/2/1/1, reduction ratios 8/4/2/1; on 2 x 3 x 64 x 96 images the stages have
384 / 96 / 24 / 6 tokens against 6 keys each.  Subnet 'sub': depths 1/1/1/1, heads 1/1/2/1, ratios 2/4/3/2.

Bounds: features, logits, losses and every active parameter's gradient at the 1e-3 max norm of the
end-to-end tests of the other backbones (tests/parity.py); gradients of inactive slices and skipped blocks
exactly zero or absent."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_mit as M
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = 64, 96


def make_backbone(seed=0):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(M.tiny_backbone_cfg())
    M.randomize_mit(m, seed)
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
        outs = M.mit_ref(sd, img.double(), M.SUBNETS[name])
        sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
        _REF[name] = ([o.detach() for o in outs], {k: v.grad for k, v in sd.items()})
    return _REF[name]


@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name):
    a = M.SUBNETS[name]
    feats_r, grads_r = reference(name)
    m = make_backbone().to(DEV).train()
    m.manipulate_arch(M.arch_of(name))
    img = make_batch(2, H, W, seed=1)[0].to(DEV)
    outs = m(img)
    assert [tuple(o.shape) for o in outs] == [(2, d, H // s, W // s) for d, s in zip(M.widths(a), (4, 8, 16, 32))]
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
        idx = M.active_slice(k, a)
        if idx is None:          # a block past the stage's depth
            assert ref is None or float(ref.abs().max()) == 0
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert got is not None, k
        outside = torch.ones(ref.shape, dtype=torch.bool)
        outside[idx] = False
        assert not bool(ref[outside].any())
        assert not bool(got.cpu()[outside].any()), "%s: gradient outside the active slice" % k
        if k.endswith("attention.k_proj.bias"):
            # softmax does not see a shift common to all keys' scores: exactly 0 in exact arithmetic and
            # rounding noise in any floating one, so the bound is absolute, TOL of the query bias's largest
            # element (tests/test_elastic_vit_gpu.py)
            bound = TOL * float(grads_r[k.replace("k_proj", "q_proj")].abs().max())
            assert float(ref.abs().max()) <= bound and float(got.abs().max()) <= bound, k
            continue
        worst[k] = rel_err(got, ref)
    w = max(worst, key=worst.get)
    print("%s: %d parameter gradients, worst %s %.3g" % (name, len(worst), w, worst[w]))
    assert worst[w] <= TOL, {k: v for k, v in worst.items() if v > TOL}
    n_sr = sum(d for d, sr in zip(a["depth"], M.TINY["sr_ratios"]) if sr > 1)
    assert len(worst) == 4 * 6 + sum(a["depth"]) * 17 + n_sr * 4
    if name == "sub":    # the slices beyond the active widths, and the skipped block
        st = m.stages
        assert float(st[1].patch_embeddings.proj.weight.grad[64:].abs().max()) == 0
        assert float(st[2].patch_embeddings.proj.weight.grad[:, 64:].abs().max()) == 0
        assert float(st[2].blocks[0].attention.q_proj.weight.grad[128:].abs().max()) == 0
        assert float(st[0].blocks[0].mlp.fc1.weight.grad[128:].abs().max()) == 0
        g = st[1].blocks[1].mlp.fc1.weight.grad
        assert g is None or float(g.abs().max()) == 0


def test_an_input_that_is_no_multiple_of_32_is_refused(hip_lib):
    m = make_backbone().to(DEV)
    with pytest.raises(ValueError, match="64 x 80"):
        m(torch.zeros(1, 3, 64, 80, device=DEV))


# ---- the head ----------------------------------------------------------------------------------------------
def conv_bn_relu_ref(sd, prefix, x, padding=0, eps=1e-5):
    """DynamicConvModule in training mode on float64: conv (no bias), BatchNorm on batch statistics, ReLU"""
    y = F.conv2d(x, sd[prefix + ".conv.weight"][:, :x.shape[1]], None, padding=padding)
    return F.relu(F.batch_norm(y, None, None, sd[prefix + ".bn.weight"], sd[prefix + ".bn.bias"], True, 0.0, eps))


def segformer_head_ref(sd, feats, align_corners, prefix=""):
    size = feats[0].shape[2:]
    outs = []
    for i, x in enumerate(feats):
        y = conv_bn_relu_ref(sd, prefix + "convs.%d" % i, x)
        outs.append(y if i == 0 else F.interpolate(y, size=size, mode="bilinear", align_corners=align_corners))
    y = conv_bn_relu_ref(sd, prefix + "fusion_conv", torch.cat(outs, dim=1))
    return F.conv2d(y, sd[prefix + "conv_seg.weight"], sd[prefix + "conv_seg.bias"])


def randomize_head(head, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in head.named_parameters():
            if ".bn." in k and k.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)


@pytest.mark.parametrize("align_corners", [False, True])
def test_segformer_head_against_float64(hip_lib, align_corners):
    """four random maps of the active widths 64 / 64 / 128 / 64 (below in_channels 64 / 128 / 192 / 128 except at
    level 0), forward and backward"""
    from gaia_seg_amd.models import build_head
    head = build_head(M.segformer_head_cfg(M.widths(M.SUBNETS["max"]), align_corners=align_corners))
    randomize_head(head, 2)
    sd = {k: v.detach().clone().double().requires_grad_(v.is_floating_point()) for k, v in head.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(2, c, H // s, W // s, generator=g)
             for c, s in zip(M.widths(M.SUBNETS["sub"]), (4, 8, 16, 32))]
    fr = [f.double().requires_grad_(True) for f in feats]
    want = segformer_head_ref(sd, fr, align_corners)
    cot = cotangents([want])[0]
    (want * cot.double()).sum().backward()
    head = head.to(DEV).train()
    fg = [f.to(DEV).requires_grad_(True) for f in feats]
    got = head(fg)
    assert tuple(got.shape) == (2, 19, H // 4, W // 4)
    assert rel_err(got, want) <= TOL
    got.backward(cot.to(DEV))
    torch.cuda.synchronize()
    for i, (a, r) in enumerate(zip(fg, fr)):
        assert rel_err(a.grad, r.grad) <= TOL, "input %d" % i
    for k, p in head.named_parameters():
        assert rel_err(p.grad, sd[k].grad) <= TOL, k
    assert float(head.convs[1].conv.weight.grad[:, 64:].abs().max()) == 0


# ---- the segmentor -----------------------------------------------------------------------------------------
def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(M.tiny_model_cfg()))
    M.randomize_mit(model.backbone, seed)
    randomize_head(model.decode_head, seed + 1)
    randomize_head(model.auxiliary_head, seed + 2)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def losses_ref(model, name, img, gt):
    """{'decode.loss_seg', 'aux.loss_seg'} of the model's weights on subnet ``name`` in float64"""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    feats = M.mit_ref({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, img.double(),
                      M.SUBNETS[name])
    logits = segformer_head_ref(sd, feats, False, "decode_head.")
    y = conv_bn_relu_ref(sd, "auxiliary_head.convs.0", feats[2], padding=1)
    aux = F.conv2d(y, sd["auxiliary_head.conv_seg.weight"], sd["auxiliary_head.conv_seg.bias"])
    out = {}
    for key, lg, wt in (("decode.loss_seg", logits, 1.0), ("aux.loss_seg", aux, 0.4)):
        up = F.interpolate(lg, size=gt.shape[2:], mode="bilinear", align_corners=False)
        # mmseg's weight_reduce_loss: the mean over ALL pixels, the ignored ones counting 0
        out[key] = wt * float(F.cross_entropy(up, gt.squeeze(1), ignore_index=255, reduction="none").mean())
    return out


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


def _train(names, graphs, monkeypatch):
    if graphs:
        monkeypatch.setenv("GS_STEP_GRAPH", "1")
    else:
        monkeypatch.delenv("GS_STEP_GRAPH", raising=False)
    model = _model()
    runner = _runner(model)
    assert runner.graphs_enabled == graphs
    runner.call_hook("before_run")
    logs = []
    for it, name in enumerate(names):
        runner.set_arch(M.arch_meta(name))
        out = runner.train_iter(_batch(it))
        logs.append({k: float(v) for k, v in out["log_vars"].items()})
    torch.cuda.synchronize()
    return model, runner, logs


def test_two_adamw_iterations_on_two_archs(hip_lib, monkeypatch):
    first = _model()
    b0 = _batch(0)
    want = losses_ref(first, "sub", b0["img"].cpu(), b0["gt_semantic_seg"].cpu())
    model, runner, logs = _train(["sub", "max"], False, monkeypatch)
    print(logs, want)
    for lg in logs:
        assert lg and all(v == v and abs(v) < 1e6 for v in lg.values()), lg
    for key in ("decode.loss_seg", "aux.loss_seg"):
        assert abs(logs[0][key] - want[key]) <= TOL * want[key], key
    assert abs(logs[0]["loss"] - sum(want.values())) <= TOL * sum(want.values())
    assert logs[1] != logs[0]
    assert getattr(model, "step_graph_capturable", True)


def test_step_graph_replay_equals_the_eager_steps(hip_lib, monkeypatch):
    """a repeated arch is captured and replayed: the same losses, bit for bit, as the eager steps"""
    names = ["sub", "sub", "sub", "sub"]
    _, r_e, logs_e = _train(names, False, monkeypatch)
    model, r_g, logs_g = _train(names, True, monkeypatch)
    assert r_e.graph_stats["replayed"] == 0 and r_g.graph_stats["captured"] == 1 and r_g.graph_stats["replayed"] >= 1
    assert logs_e == logs_g


def test_whole_and_slide_evaluation(hip_lib):
    from gaia_seg_amd.core.config import ConfigDict
    model = _model().eval()
    img = make_batch(1, 2 * H, 2 * W, seed=5)[0].to(DEV)
    metas = [dict(ori_shape=(2 * H, 2 * W, 3), img_shape=(2 * H, 2 * W, 3), flip=False)]
    with torch.no_grad():
        whole = model.inference(img, metas, rescale=False)
        assert tuple(whole.shape) == (1, 19, 2 * H, 2 * W) and bool(torch.isfinite(whole).all())
        model.test_cfg = ConfigDict(mode="slide", crop_size=(H, W), stride=(H, W))
        probs = model.inference(img, metas, rescale=False)
        for y0 in (0, H):
            for x0 in (0, W):
                want = model.encode_decode(img[:, :, y0:y0 + H, x0:x0 + W].contiguous(), None).softmax(dim=1)
                assert rel_err(probs[:, :, y0:y0 + H, x0:x0 + W], want) <= 3e-5, (y0, x0)
        labels = model.simple_test_device(img, metas, rescale=True)
    assert tuple(labels.shape) == (1, 2 * H, 2 * W) and labels.dtype == torch.int64
