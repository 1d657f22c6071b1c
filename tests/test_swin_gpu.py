"""DynamicSwinTransformer and the UPerNet segmentor it makes, on the GPU against the float64 restatement of
tests/util_swin.py carrying the same weights (which tests/test_swin.py ties to transformers' SwinBackbone).  The
tiny supernet: window 7, depths 2/2/2/1, heads 2/2/3/2 (widths 64/64/96/64).  On 2 x 3 x 64 x 96 images the maps are
16x24, 8x12, 4x6 and 2x3: every stage pads, two stages are smaller than a window, odd blocks shift.  On 224 x 224
no stage pads.  Subnet 'sub': depths 1/2/1/1, heads 1/2/2/1, ratios 4/2/3/4.

Bounds: features and every active parameter's gradient at the 1e-3 max norm of tests/test_mit_gpu.py; gradients
of skipped blocks and of swin.layernorm absent or exactly zero."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_swin as S
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = 64, 96


def make_backbone(seed=0):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(S.tiny_backbone_cfg())
    S.randomize_swin(m, seed)
    return m


def arch_of(name):
    return {"body": copy.deepcopy(S.SUBNETS[name])}


def arch_meta(name):
    a = S.SUBNETS[name]
    return {"name": name, "arch.backbone.body.depth": list(a["depth"]),
            "arch.backbone.body.num_heads": list(a["num_heads"]), "arch.backbone.body.mlp_ratio": list(a["mlp_ratio"])}


def cotangents(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(o.shape, generator=g) for o in outs]


_REF = {}


def reference(name, h=H, w=W, n=2):
    """(features, {state-dict key: gradient}) of subnet ``name`` in float64, computed once per session"""
    key = (name, h, w)
    if key not in _REF:
        m = make_backbone()
        sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
        img = make_batch(n, h, w, seed=1)[0]
        outs = S.swin_ref(sd, img.double(), S.SUBNETS[name])
        sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
        _REF[key] = ([o.detach() for o in outs], {k: v.grad for k, v in sd.items()})
    return _REF[key]


def state_dict_layout(name, grad):
    """a parameter's gradient in the layout of its state-dict entry"""
    if name.endswith("downsample.reduction.weight"):
        return grad.permute(0, 3, 2, 1).reshape(grad.shape[0], -1)
    if grad.dim() == 4 and grad.shape[2:] == (1, 1):
        return grad[:, :, 0, 0]
    return grad


@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name):
    a = S.SUBNETS[name]
    feats_r, grads_r = reference(name)
    m = make_backbone().to(DEV).train()
    m.manipulate_arch(arch_of(name))
    img = make_batch(2, H, W, seed=1)[0].to(DEV)
    outs = m(img)
    assert [tuple(o.shape) for o in outs] == [(2, 32 * hd, H // s, W // s)
                                              for hd, s in zip(a["num_heads"], (4, 8, 16, 32))]
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        err = rel_err(o, r)
        print("%s: feature %d rel_err %.3g" % (name, i, err))
        assert err <= TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    check_gradients(m, grads_r, a, name)


def check_gradients(m, grads_r, a, name):
    """every active parameter's gradient within TOL of float64, nothing on inactive parameters or slices"""
    worst, active = {}, {id(p) for mod in m.active_modules() for p in mod.parameters()}
    for k, p in m.named_parameters():
        ref = grads_r[k]
        got = None if p.grad is None else state_dict_layout(k, p.grad.cpu())
        if ref is None or float(ref.abs().max()) == 0:          # a skipped block, swin.layernorm
            assert id(p) not in active, k
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert id(p) in active and got is not None, k
        if k.endswith("attention.k_proj.bias"):
            # softmax does not see a shift common to all keys' scores: exactly 0 in exact arithmetic and rounding
            # noise in any floating one, so the bound is absolute (tests/test_mit_gpu.py)
            bound = TOL * float(grads_r[k.replace("k_proj", "q_proj")].abs().max())
            assert float(ref.abs().max()) <= bound and float(got.abs().max()) <= bound, k
            continue
        assert not bool(got[ref == 0].any()), "%s: gradient outside the active slice" % k
        worst[k] = rel_err(got, ref)
    w = max(worst, key=worst.get)
    print("%s: %d parameter gradients, worst %s %.3g" % (name, len(worst), w, worst[w]))
    assert worst[w] <= TOL, {k: v for k, v in worst.items() if v > TOL}
    # embeddings 4, per block 17 - 1 (k_proj.bias), per merge 3, four output norms
    assert len(worst) == 4 + sum(a["depth"]) * 16 + 3 * 3 + 8
    assert "swin.layernorm.weight" not in worst


def test_no_pad_or_crop_launch_when_no_stage_pads(hip_lib, monkeypatch):
    """1 x 224 x 224: the maps are 56, 28, 14 and 7, all multiples of the window -- features of MAX at 1e-3, features
    and every gradient of the depth-1 subnet at 1e-3 (q / k / v straight from LN(x), the attention's output straight
    into o_proj), and neither ops.map_pad nor ops.map_crop is called; at 64 x 96 every block calls both"""
    from gaia_seg_amd.hip import ops
    calls = {"pad": 0, "crop": 0}
    pad, crop = ops.map_pad, ops.map_crop
    monkeypatch.setattr(ops, "map_pad", lambda *a, **k: (calls.__setitem__("pad", calls["pad"] + 1), pad(*a, **k))[1])
    monkeypatch.setattr(ops, "map_crop", lambda *a, **k: (calls.__setitem__("crop", calls["crop"] + 1), crop(*a, **k))[1])
    m = make_backbone().to(DEV).eval()
    feats_r, _ = reference("max", 224, 224, 1)
    with torch.no_grad():
        outs = m(make_batch(1, 224, 224, seed=1)[0].to(DEV))
    assert calls == {"pad": 0, "crop": 0}
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        assert rel_err(o, r) <= TOL, i
    feats_r, grads_r = reference("sub", 224, 224, 1)
    m.train()
    m.manipulate_arch(arch_of("sub"))
    outs = m(make_batch(1, 224, 224, seed=1)[0].to(DEV))
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        assert rel_err(o, r) <= TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    assert calls == {"pad": 0, "crop": 0}
    check_gradients(m, grads_r, S.SUBNETS["sub"], "sub at 224")
    m.manipulate_arch(m.full_arch_meta())
    with torch.no_grad():
        m(make_batch(2, H, W, seed=1)[0].to(DEV))
    assert calls == {"pad": 7, "crop": 7}


def test_an_input_that_is_no_multiple_of_32_is_refused(hip_lib):
    m = make_backbone().to(DEV)
    with pytest.raises(ValueError, match="64 x 80"):
        m(torch.zeros(1, 3, 64, 80, device=DEV))


# ---- the segmentor -----------------------------------------------------------------------------------------
def tiny_model_cfg():
    """DynamicUPerHead on the tiny Swin supernet, with the FCN auxiliary head on stage 3"""
    from util_models import fcn_head, uper_head
    widths = [32 * h for h in S.TINY["num_heads"]]
    return dict(type="DynamicEncoderDecoder", backbone=S.tiny_backbone_cfg(),
                decode_head=uper_head(in_channels=widths, channels=16),
                auxiliary_head=fcn_head(in_channels=widths[2], in_index=2, channels=16, num_convs=1,
                                        concat_input=False, loss_weight=0.4),
                train_cfg=dict(), test_cfg=dict(mode="whole"))


def randomize_head(head, seed):
    """the heads away from their init, as tests/test_mit_gpu.py does it"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in head.named_parameters():
            if ".bn." in k and k.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)


def conv_bn_relu_ref(sd, prefix, x, padding=0, eps=1e-5):
    """DynamicConvModule in training mode on float64: conv (no bias) on the leading input channels, BatchNorm on
    batch statistics, ReLU"""
    y = F.conv2d(x, sd[prefix + ".conv.weight"][:, :x.shape[1]], None, padding=padding)
    return F.relu(F.batch_norm(y, None, None, sd[prefix + ".bn.weight"], sd[prefix + ".bn.bias"], True, 0.0, eps))


def uper_head_ref(sd, feats, prefix, pool_scales=(1, 2, 3, 6)):
    """mmseg's UPerHead on float64 NCHW features: the pooling pyramid on the last level, 1x1 laterals, the
    top-down bilinear sums, 3x3 fpn convs, everything resized to level 0, the 3x3 fusion, conv_seg"""
    def up(t, size):
        return F.interpolate(t, size=size, mode="bilinear", align_corners=False)
    x = feats[-1]
    pyramid = [x] + [up(conv_bn_relu_ref(sd, prefix + "psp_modules.%d.1" % i, F.adaptive_avg_pool2d(x, s)), x.shape[2:])
                     for i, s in enumerate(pool_scales)]
    laterals = [conv_bn_relu_ref(sd, prefix + "lateral_convs.%d" % i, f) for i, f in enumerate(feats[:-1])]
    laterals.append(conv_bn_relu_ref(sd, prefix + "bottleneck", torch.cat(pyramid, dim=1), padding=1))
    for i in range(len(laterals) - 1, 0, -1):
        laterals[i - 1] = laterals[i - 1] + up(laterals[i], laterals[i - 1].shape[2:])
    outs = [conv_bn_relu_ref(sd, prefix + "fpn_convs.%d" % i, laterals[i], padding=1) for i in range(len(laterals) - 1)]
    outs.append(laterals[-1])
    size = outs[0].shape[2:]
    y = torch.cat([outs[0]] + [up(o, size) for o in outs[1:]], dim=1)
    y = conv_bn_relu_ref(sd, prefix + "fpn_bottleneck", y, padding=1)
    return F.conv2d(y, sd[prefix + "conv_seg.weight"], sd[prefix + "conv_seg.bias"])


def losses_ref(model, name, img, gt):
    """{'decode.loss_seg', 'aux.loss_seg'} of the model's weights on subnet ``name`` in float64"""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    feats = S.swin_ref({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, img.double(),
                       S.SUBNETS[name])
    logits = uper_head_ref(sd, feats, "decode_head.")
    y = conv_bn_relu_ref(sd, "auxiliary_head.convs.0", feats[2], padding=1)
    aux = F.conv2d(y, sd["auxiliary_head.conv_seg.weight"], sd["auxiliary_head.conv_seg.bias"])
    out = {}
    for key, lg, wt in (("decode.loss_seg", logits, 1.0), ("aux.loss_seg", aux, 0.4)):
        up = F.interpolate(lg, size=gt.shape[2:], mode="bilinear", align_corners=False)
        # mmseg's weight_reduce_loss: the mean over ALL pixels, the ignored ones counting 0
        out[key] = wt * float(F.cross_entropy(up, gt.squeeze(1), ignore_index=255, reduction="none").mean())
    return out


def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(tiny_model_cfg()))
    S.randomize_swin(model.backbone, seed)
    randomize_head(model.decode_head, seed + 1)
    randomize_head(model.auxiliary_head, seed + 2)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _runner(model):
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
        runner.set_arch(arch_meta(name))
        out = runner.train_iter(_batch(it))
        logs.append({k: float(v) for k, v in out["log_vars"].items()})
    torch.cuda.synchronize()
    return model, runner, logs


def test_two_adamw_iterations_on_two_archs(hip_lib, monkeypatch):
    """two AdamW steps of the tiny UPerNet segmentor on two archs: the first step's losses equal the float64
    model's (swin_ref, a float64 UPerHead and FCN head, mmseg's loss reduction) at 1e-3; finite, different losses;
    the unread swin.layernorm keeps its value"""
    before = _model()
    b0 = _batch(0)
    want = losses_ref(before, "sub", b0["img"].cpu(), b0["gt_semantic_seg"].cpu())
    model, runner, logs = _train(["sub", "max"], False, monkeypatch)
    print(logs, want)
    for lg in logs:
        assert lg and all(v == v and abs(v) < 1e6 for v in lg.values()), lg
    for key in ("decode.loss_seg", "aux.loss_seg"):
        assert abs(logs[0][key] - want[key]) <= TOL * want[key], key
    assert abs(logs[0]["loss"] - sum(want.values())) <= TOL * sum(want.values())
    assert logs[1] != logs[0]
    assert getattr(model, "step_graph_capturable", True)
    sd0, sd1 = before.state_dict(), model.state_dict()
    assert torch.equal(sd0["backbone.swin.layernorm.weight"], sd1["backbone.swin.layernorm.weight"])
    moved = "backbone.swin.encoder.layers.0.blocks.0.attention.relative_position_bias.relative_position_bias_table"
    assert not torch.equal(sd0[moved], sd1[moved])


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
