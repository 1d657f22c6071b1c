"""The ElasticConvformer backbone on the GPU against the float64 CPU model of tests/util_convformer.py carrying
the same weights: a tiny supernet (stem 16, conv widths [32, 64, 128], embed_dim 128, 2 heads, ratio 4,
body_depth [2, 2, 2], depth 9, patch 16) on 2 x 3 x 64 x 96 images (24 tokens + cls, last map 2 x 3) and its
subnets 'max' and 'sub' (widths [16, 32, 64], D = 64, heads [1, 2, 1], depths [1, 2, 1], ratios [30, 40, 35]; depth
1 in stage 1 runs the first block only, which has no coupling unit), each with norm_eval on and off.

Bounds: features and every active parameter's gradient at TOL = 1e-3 (BASELINE.json), per parameter relative
to its largest reference gradient; the frozen stem and everything outside the active slices get no gradient.

The comparison needs the fp32 pass and the float64 pass to take the same branch of every ReLU.  The test
asserts, on the float64 pass alone, that no ReLU input lies within 1e-4 rms of zero.  That is a condition on
the inputs.  No seed satisfies it (the four passes see about a million ReLU inputs, of which any seed puts
some 80 inside that margin), so the parameters of record are made to satisfy it:
tests/golden/make_convformer_relu_margin.py moves 29 BatchNorm biases by a few 1e-4 rms, consulting the
float64 model only, and util_convformer.randomize_convformer applies the recorded values."""
import copy
import os
import sys

import pytest
import torch

from conftest import rel_err
import util_convformer as U
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = U.H, U.W
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "configs", "supernet", "upernet_elastic_convformer_adamw.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_backbone(**kw):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(U.tiny_backbone_cfg(**kw))
    U.randomize_convformer(m)
    return m


def cotangents(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(o.shape, generator=g) for o in outs]


_REF = {}


def reference(name, norm_eval):
    """(features, {parameter: gradient}) of subnet ``name`` in float64, computed once per session; asserts
    the ReLU margin on the way"""
    if (name, norm_eval) not in _REF:
        m = make_backbone()
        params = {k for k, _ in m.named_parameters()}
        sd = {k: v.detach().clone().double().requires_grad_(k in params) for k, v in m.state_dict().items()}
        img = make_batch(2, H, W, seed=U.IMG_SEED)[0]
        pre = []
        outs = U.convformer_ref(sd, img.double(), U.SUBNETS[name], norm_eval, relu_inputs=pre)
        U.assert_relu_margin(pre)
        sum((o * c.double()).sum() for o, c in zip(outs, cotangents(outs))).backward()
        _REF[name, norm_eval] = ([o.detach() for o in outs], {k: sd[k].grad for k in params})
    return _REF[name, norm_eval]


@pytest.mark.parametrize("norm_eval", [True, False], ids=["norm_eval", "batch_stats"])
@pytest.mark.parametrize("name", ["max", "sub"])
def test_features_and_gradients_against_float64(hip_lib, name, norm_eval):
    a = U.SUBNETS[name]
    feats_r, grads_r = reference(name, norm_eval)
    m = make_backbone(norm_eval=norm_eval).to(DEV).train()
    m.manipulate_arch(U.arch_of(name))
    img = make_batch(2, H, W, seed=U.IMG_SEED)[0].to(DEV)
    outs = m(img)
    w = a["widths"]
    assert [tuple(o.shape) for o in outs] == [(2, w[0], 16, 24), (2, w[1], 8, 12), (2, w[2], 4, 6), (2, w[2], 2, 3)]
    for i, (o, r) in enumerate(zip(outs, feats_r)):
        err = rel_err(o, r)
        print("%s: feature %d rel_err %.3g" % (name, i, err))
        assert err <= TOL, i
    torch.autograd.backward(list(outs), [c.to(DEV) for c in cotangents(outs)])
    torch.cuda.synchronize()
    worst, vanishing = {}, []
    for k, p in m.named_parameters():
        ref, got = grads_r[k], p.grad
        if k.startswith(("conv1.", "bn1.")):     # the frozen stem
            assert not p.requires_grad and (got is None or float(got.abs().max()) == 0), k
            continue
        if got is not None and ref is not None and ref.dim() == 2:
            got = got[:, :, 0, 0]                                # a linear weight: [out, in] in the state dict
        idx = U.active_slice(k, a)
        if idx is None:          # a skipped block, the relative-position tables
            assert ref is None or float(ref.abs().max()) == 0
            assert got is None or float(got.abs().max()) == 0, "%s: gradient on an inactive parameter" % k
            continue
        assert got is not None, k
        outside = torch.ones(ref.shape, dtype=torch.bool)
        outside[idx] = False
        assert not bool(ref[outside].any())
        assert not bool(got.cpu()[outside].any()), "%s: gradient outside the active slice" % k
        if k.endswith("attn.w_ks.bias"):
            # softmax does not see a shift common to all keys' scores, so this gradient is exactly 0 in exact
            # arithmetic and rounding noise in any floating one: the bound is absolute, TOL of the query
            # bias's largest element (tests/test_elastic_vit_gpu.py)
            bound = TOL * float(grads_r[k.replace("w_ks", "w_qs")].abs().max())
            assert float(ref.abs().max()) <= bound and float(got.abs().max()) <= bound, k
            continue
        if k.endswith(".bias") and not norm_eval:
            # With batch statistics some bias gradients are exactly 0 in exact arithmetic, and rounding noise
            # in float64 as in fp32: a bias gradient is the plain sum of the gradient in front of its layer,
            # and a shift that is constant over a channel is removed by a batch-statistics BatchNorm behind it
            # (the conv bias in front of expand_block.bn1; the output bias of the last transformer block, whose
            # tokens feed only that projection; a BatchNorm bias whose channel passes its ReLU everywhere and
            # feeds only convs followed by such BatchNorms, as cnn_block.bn3 of stage 4 does).  There is no
            # relative error to take.  The same gradient enters the weight sibling's gradient multiplied by
            # O(1) activations, without cancelling, so the bound is absolute: TOL of that sibling's largest
            # reference element.  The rule looks at the float64 gradients only.
            bound = TOL * float(grads_r[k[:-4] + "weight"].abs().max())
            if float(ref.abs().max()) <= bound:
                assert float(got.abs().max()) <= bound, k
                vanishing.append(k)
                continue
        worst[k] = rel_err(got, ref)
    top = max(worst, key=worst.get)
    print("%s: %d parameter gradients, worst %s %.3g; %d vanish: %s" % (name, len(worst), top, worst[top],
                                                                        len(vanishing), vanishing))
    print({k: "%.3g" % v for k, v in worst.items() if v > TOL})
    assert worst[top] <= TOL, {k: v for k, v in worst.items() if v > TOL}
    assert all(k.endswith("expand_block.conv_project.bias") or k in ("conv_trans_4.0.cnn_block.bn3.bias",
                                                                       "conv_trans_4.0.trans_block.mlp.layer2.bias")
               for k in vanishing), vanishing
    assert norm_eval or sum(k.endswith("expand_block.conv_project.bias") for k in vanishing) == sum(a["depths"])
    for k in ("cls_token", "conv_trans_1.0.trans_patch_conv.weight", "conv_trans_2.1.squeeze_block.ln1.weight",
              "conv_trans_2.1.squeeze_block.conv_project.bias", "conv_trans_4.0.expand_block.bn1.weight",
              "conv_trans_4.0.expand_block.conv_project.weight", "conv_trans_4.0.fusion_block.conv2.weight"):
        assert k in worst, k
    # of the 323 parameters: all but the stem (3), 28 relative-position tables and 7 key biases at 'max';
    # 'sub' also leaves out its two skipped blocks
    assert len(worst) + len(vanishing) == {"max": 285, "sub": 203}[name]
    if name == "sub":    # the slices beyond the active widths, and the skipped blocks
        assert float(m.cls_token.grad[..., 64:].abs().max()) == 0
        assert float(m.conv_trans_2[0].squeeze_block.ln1.weight.grad[64:].abs().max()) == 0
        assert float(m.conv_trans_2[0].expand_block.conv_project.weight.grad[8:].abs().max()) == 0
        assert float(m.conv_trans_2[0].expand_block.conv_project.weight.grad[:, 64:].abs().max()) == 0
        g = m.conv_trans_1[1].cnn_block.conv1.weight.grad
        assert g is None or float(g.abs().max()) == 0


def test_an_input_that_is_no_multiple_of_twice_the_patch_is_refused(hip_lib):
    m = make_backbone().to(DEV)
    with pytest.raises(ValueError, match="img_size"):
        m(torch.zeros(1, 3, 64, 80, device=DEV))


def _model(seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(U.tiny_model_cfg()))
    U.randomize_convformer(model.backbone)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _runner(model):
    """the optimizer of the config of record; of its schedule only the poly decay (at iteration 0 its
    warm-up scales the step by 1e-6, below one ulp of most parameters: nothing would move)"""
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, PolyLrUpdaterHook
    optimizer = Config.fromfile(CONFIG).optimizer
    opt = check_optimizer_cfg(optimizer)
    assert opt["type"] == "AdamW"
    arena = ParamArena(model)
    arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    pg = build_param_groups(model, optimizer)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=0.0, weight_decay=opt["weight_decay"], max_iters=100, param_groups=pg)
    runner.register_hook(PolyLrUpdaterHook(power=1.0, min_lr=0.0, by_epoch=False))
    runner.register_hook(ArenaOptimizerHook())
    return runner, pg


def _batch(seed):
    img, gt = make_batch(2, H, W, seed=seed)
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False) for _ in range(2)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def _one_step():
    model = _model()
    runner, pg = _runner(model)
    runner.call_hook("before_run")
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner.set_arch(U.arch_meta("sub"))
    out = runner.train_iter(_batch(0))
    torch.cuda.synchronize()
    return model, before, {k: float(v) for k, v in out["log_vars"].items()}, pg


def test_one_adamw_step_moves_the_active_unfrozen_parameters_only_and_repeats_bit_for_bit(hip_lib):
    model, before, logs, pg = _one_step()
    assert logs and all(v == v and abs(v) < 1e6 for v in logs.values()), logs
    assert len(pg) == 2                      # decayed; undecayed (norms and cls_token)
    undecayed = set(pg.members(1))
    assert "backbone.cls_token" in undecayed and "backbone.conv_trans_2.0.squeeze_block.ln1.weight" in undecayed
    assert "backbone.conv_trans_2.0.expand_block.bn1.bias" in undecayed
    assert "backbone.conv_trans_2.0.expand_block.conv_project.bias" not in undecayed
    after = dict(model.named_parameters())
    active = {id(p) for p in model.active_parameters()}
    n_active = n_idle = 0
    for k, p in after.items():
        moved = not torch.equal(p, before[k])
        if id(p) in active and p.requires_grad:
            assert moved, "%s is active and did not change" % k
            n_active += 1
        else:
            assert not moved, "%s is inactive or frozen and changed" % k
            n_idle += 1
    idle = [k for k, p in after.items() if id(p) not in active or not p.requires_grad]
    assert "backbone.conv1.weight" in idle and "backbone.bn1.bias" in idle
    assert any(k.startswith("backbone.conv_trans_1.1.") for k in idle)
    assert any(k.startswith("backbone.conv_trans_3.1.") for k in idle)
    assert any("rel_pos_embed" in k for k in idle)
    assert n_active > 150 and n_idle > 100
    # the same step from the same snapshot
    model2, before2, logs2, _ = _one_step()
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
    assert [len(getattr(bb, n)) for n in bb.layers] == a["depths"] + [1]
    sd = bb.state_dict()
    assert tuple(sd["cls_token"].shape) == (1, 1, 64)
    assert tuple(sd["conv_trans_1.0.trans_patch_conv.weight"].shape) == (64, 16, 4, 4)
    assert tuple(sd["conv_trans_1.0.conv_1.conv2.weight"].shape) == (4, 4, 3, 3)
    assert tuple(sd["conv_trans_2.0.cnn_block.residual_conv.weight"].shape) == (32, 16, 1, 1)
    assert tuple(sd["conv_trans_2.1.squeeze_block.conv_project.weight"].shape) == (64, 8, 1, 1)
    assert tuple(sd["conv_trans_2.1.squeeze_block.ln1.weight"].shape) == (64,)
    assert tuple(sd["conv_trans_2.1.expand_block.conv_project.weight"].shape) == (8, 64, 1, 1)
    assert tuple(sd["conv_trans_2.1.expand_block.bn1.running_var"].shape) == (8,)
    assert tuple(sd["conv_trans_2.0.trans_block.attn.w_qs.weight"].shape) == (128, 64)
    assert tuple(sd["conv_trans_3.0.trans_block.mlp.layer1.weight"].shape) == (224, 64)
    assert tuple(sd["conv_trans_4.0.trans_block.mlp.layer2.weight"].shape) == (64, 224)
    assert tuple(sd["conv_trans_4.0.fusion_block.conv3.weight"].shape) == (64, 16, 1, 1)
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
