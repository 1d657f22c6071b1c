"""``fp16_attention`` on the backbones, on the tiny supernet of tests/util_vit.py and
the tiny BEiT of tests/util_beit.py.

The tolerance rule: switching the attention to fp16 operands inside an fp16 mode may change a result by at
most FACTOR = 3 times what the fp16 mode itself changed it by (against fp32) -- the attention rounds the
same activations to the same format as the linears around it; the factor is the one of the operator tests
(tests/util_attention_f16.py).

Recorded on one MI355X: profiles/r19_fp16_attention.md."""
import contextlib
import copy

import pytest
import torch

from conftest import rel_err
import util_vit as U
from test_adamw_gpu import OPTIMIZER, _batch, _meta, _model, _runner
from test_attention_f16_gpu import Counter
from test_beit_gpu import make_backbone as make_beit
from test_elastic_vit_gpu import make_backbone
from util_attention_f16 import FACTOR
from util_models import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = U.TINY["img_size"]


def features(m, img, precision, hip_lib):
    """-> (feature maps, the attention entries called) of an eval forward under forward_precision"""
    from gaia_seg_amd.hip import ops
    scope = ops.forward_precision("fp16") if precision == "fp16" else contextlib.nullcontext()
    with torch.no_grad(), scope, Counter(hip_lib) as cnt:
        outs = m(img)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], cnt.used()


def worst(a, b):
    return max(rel_err(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["max", "sub"])
def test_backbone_features_with_and_without_the_flag(hip_lib, name):
    layers = sum(U.SUBNETS[name]["layers"])
    m = make_backbone().to(DEV).eval()
    assert m.fp16_attention is False
    m.manipulate_arch(U.arch_of(name))
    img = make_batch(2, H, W, seed=1)[0].to(DEV)
    f32, used = features(m, img, "fp32", hip_lib)
    assert used == {"forward": layers}
    f16, used = features(m, img, "fp16", hip_lib)
    assert used == {"forward": layers}, "the flag is off: no fp16 attention entry may run"
    m.fp16_attention = False   # set explicitly: the same as left alone
    again, _ = features(m, img, "fp16", hip_lib)
    for a, b in zip(f16, again):
        assert torch.equal(a, b)
    m.fp16_attention = True
    flagged32, used = features(m, img, "fp32", hip_lib)
    assert used == {"forward": layers}, "outside an fp16 mode the flag does nothing"
    for a, b in zip(f32, flagged32):
        assert torch.equal(a, b)
    f16a, used = features(m, img, "fp16", hip_lib)
    assert used == {"forward_f16": layers}, "one fp16 entry per active layer, none for a skipped one: %s" % used
    d_conv, d_attn = worst(f16, f32), worst(f16a, f16)
    print("%s: d_conv %.3e d_attn %.3e ratio %.2f" % (name, d_conv, d_attn, d_attn / d_conv))
    assert d_attn > 0, "the fp16 attention changed nothing"
    assert d_attn <= FACTOR * d_conv


def one_step(mode):
    """one AdamW runner step on the 'sub' arch -> (model, parameters before, log_vars, unscaled flat gradient);
    mode: 'fp32', 'fp16' (Fp16OptimizerHook(loss_scale=512.)) or 'fp16+attention' (plus fp16.attention)"""
    from gaia_seg_amd.apis.train import optimizer_hook
    model = _model("vit")
    oc = None if mode == "fp32" else dict(type="Fp16OptimizerHook", loss_scale=512.)
    fp16 = dict(attention=True) if mode == "fp16+attention" else None
    runner, arena, _ = _runner(model, hook=optimizer_hook(oc, fp16))
    grad = torch.zeros_like(arena.flat_grad)
    orig = arena.adamw_step

    def recorded(ranges, lr, weight_decay, grad_scale=1.0, zero_grad=False, hyper=None):
        for a, b in ranges:
            grad[a:b] = arena.flat_grad[a:b] * grad_scale
        return orig(ranges, lr, weight_decay, grad_scale, zero_grad, hyper=hyper)
    arena.adamw_step = recorded
    runner.call_hook("before_run")
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner.set_arch(_meta("vit", "sub"))
    out = runner.train_iter(_batch("vit", 0))
    torch.cuda.synchronize()
    return model, before, {k: float(v) for k, v in out["log_vars"].items()}, grad.cpu()


def test_one_fp16_runner_step_with_fp16_attention(hip_lib):
    assert OPTIMIZER["type"] == "AdamW"
    with Counter(hip_lib) as cnt:
        model, before, logs, g_on = one_step("fp16+attention")
    layers = sum(U.SUBNETS["sub"]["layers"])
    assert cnt.used() == {"forward_f16": layers, "backward_f16": layers}, cnt.used()
    assert model.backbone.fp16_attention is True and model.fp16_enabled is True
    assert logs and all(v == v and abs(v) < 1e6 for v in logs.values()), logs
    assert bool(torch.isfinite(g_on).all())
    active = {id(p) for p in model.active_parameters()}
    for k, p in model.named_parameters():
        assert (not torch.equal(p, before[k])) == (id(p) in active), \
            "%s: active parameters move, inactive ones do not" % k
    model2, before2, logs2, g_again = one_step("fp16+attention")
    assert logs2 == logs and torch.equal(g_again, g_on)
    for (k, p), q in zip(model2.named_parameters(), model.parameters()):
        assert torch.equal(before2[k], before[k]) and torch.equal(p, q), "%s differs between two identical steps" % k
    with Counter(hip_lib) as cnt:
        g_off = one_step("fp16")[3]
    assert cnt.used() == {"forward": layers, "backward": layers}, cnt.used()
    g_32 = one_step("fp32")[3]
    d_conv, d_attn = rel_err(g_off, g_32), rel_err(g_on, g_off)
    print("gradients: d_conv %.3e d_attn %.3e ratio %.2f" % (d_conv, d_attn, d_attn / d_conv))
    assert d_attn > 0
    assert d_attn <= FACTOR * d_conv


def test_beit_features_with_the_flag(hip_lib):
    from util_beit import tiny_cfg
    variant = "p8-block-tables"   # a 4 x 6 window: 25 tokens
    h, w = tiny_cfg(variant)["img_size"]
    m = make_beit(variant).to(DEV)
    depth = len(m.blocks)
    img = make_batch(2, h, w, seed=1)[0].to(DEV)
    f32, used = features(m, img, "fp32", hip_lib)
    assert used == {"relpos_forward": depth}
    f16, used = features(m, img, "fp16", hip_lib)
    assert used == {"relpos_forward": depth}
    m.fp16_attention = True
    assert all(b.attn.fp16_attention for b in m.blocks)
    f16a, used = features(m, img, "fp16", hip_lib)
    assert used == {"relpos_forward_f16": depth}, used
    d_conv, d_attn = worst(f16, f32), worst(f16a, f16)
    print("BEiT %s: d_conv %.3e d_attn %.3e ratio %.2f" % (variant, d_conv, d_attn, d_attn / d_conv))
    assert d_attn > 0
    assert d_attn <= FACTOR * d_conv
    m2 = copy.deepcopy(m)
    assert m2.fp16_attention is True
