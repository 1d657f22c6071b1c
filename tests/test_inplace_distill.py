"""In-place distillation (sandwich rule) without a GPU: the reference's loss restated in torch and its
known answers, the sandwich sampler of the CLI / config, the head combinations that are refused, and
host-side argument checks of the new C-ABI entry points."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gaia_seg_amd.hip import lib  # noqa: E402


def kd_restated(s, t, T=2.0, weight=0.5, divisor=1000.0, interpolation=False, size=None,
                align_corners=False):
    """dynamic_psp_head.py:204-241 written from the formula: weight * mean_n(sum_{c,h,w}
    -softmax(t/T) * log softmax(s/T)) / D (log softmax as s/T - lse, the port's numerics)."""
    if interpolation:
        s = F.interpolate(s, size=size, mode="bilinear", align_corners=align_corners)
        t = F.interpolate(t, size=size, mode="bilinear", align_corners=align_corners)
    q = torch.softmax(t / T, dim=1)
    logp = torch.log_softmax(s / T, dim=1)
    return weight * (-(q * logp)).sum(dim=(1, 2, 3)).mean() / divisor


def test_identical_logits_give_the_scaled_entropy():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 19, 5, 7, generator=g, dtype=torch.float64)
    q = torch.softmax(x / 2, dim=1)
    entropy = -(q * q.log()).sum(dim=(1, 2, 3)).mean()
    assert torch.allclose(kd_restated(x, x), 0.5 * entropy / 1000, rtol=1e-12)
    # uniform logits: every pixel contributes log(C)
    z = torch.zeros(2, 19, 5, 7, dtype=torch.float64)
    assert math.isclose(float(kd_restated(z, z, weight=1.0, divisor=1.0)), 35 * math.log(19), rel_tol=1e-12)
    # a sum over pixels, a mean over the batch only
    z1 = torch.zeros(1, 19, 5, 7, dtype=torch.float64)
    assert math.isclose(float(kd_restated(z1, z1)), float(kd_restated(z, z)), rel_tol=1e-12)


def test_temperature_scales_the_logits():
    g = torch.Generator().manual_seed(1)
    s = torch.randn(2, 7, 4, 4, generator=g, dtype=torch.float64)
    t = torch.randn(2, 7, 4, 4, generator=g, dtype=torch.float64)
    for T in (1.0, 2.0, 4.0):
        assert torch.allclose(kd_restated(s * T, t * T, T=T), kd_restated(s, t, T=1.0), rtol=1e-12)
    # cross entropy >= entropy of the teacher (Gibbs), equality iff s == t
    q = torch.softmax(t / 2, dim=1)
    ent = 0.5 * (-(q * q.log())).sum(dim=(1, 2, 3)).mean() / 1000
    assert float(kd_restated(s, t)) > float(ent)


def test_divisor_and_teacher_key_per_head_class():
    from gaia_seg_amd.models.decode_heads.dynamic_fcn_head import DynamicFCNHead
    from gaia_seg_amd.models.decode_heads.dynamic_psp_head import DynamicPSPHead
    from gaia_seg_amd.models.decode_heads.dynamic_uper_head import DynamicUPerHead
    assert (DynamicPSPHead.kd_teacher_key, DynamicPSPHead.kd_divisor) == ("teacher_logits", 1000.0)
    assert (DynamicFCNHead.kd_teacher_key, DynamicFCNHead.kd_divisor) == ("aux_teacher_logits", 2000.0)
    assert DynamicUPerHead.kd_teacher_key is None
    g = torch.Generator().manual_seed(2)
    s = torch.randn(2, 19, 4, 6, generator=g, dtype=torch.float64)
    t = torch.randn(2, 19, 4, 6, generator=g, dtype=torch.float64)
    assert torch.allclose(kd_restated(s, t, divisor=1000.0), 2 * kd_restated(s, t, divisor=2000.0))


def test_reference_defaults():
    from gaia_seg_amd.models.losses.distill_loss import KD_DEFAULTS
    assert KD_DEFAULTS == dict(T=2.0, distillation_weight=0.5, interpolation=False)


def _cfg(**kw):
    from gaia_seg_amd.core.config import Config
    base = dict(
        max_net=dict(type="anchor", anchors=[{"name": "MAX", "arch.backbone.stem.width": 32}]),
        min_net=dict(type="anchor", anchors=[{"name": "MIN", "arch.backbone.stem.width": 16}]),
        random_subnet=dict(type="range", key="arch.backbone.stem.width", start=16, end=32, step=8))
    base.update(kw)
    return Config({k: v for k, v in base.items() if v is not None})


def test_sandwich_sampler_order_and_count():
    from gaia_seg_amd.apis import sandwich_train_sampler
    from gaia_seg_amd.core.model_space import build_model_sampler
    for num, cfg in ((3, _cfg()), (1, _cfg(sample_subnet_num=1)), (5, _cfg(sample_subnet_num=5))):
        s = build_model_sampler(sandwich_train_sampler(cfg))
        s.seed(0)
        for _ in range(3):
            members = s.candidates()
            assert len(members) == 2 + num
            assert members[0]["name"] == "MAX" and members[1]["name"] == "MIN"
            assert all("name" not in m and m["arch.backbone.stem.width"] in (16, 24, 32)
                       for m in members[2:])


@pytest.mark.parametrize("missing", ["max_net", "min_net", "random_subnet"])
def test_sandwich_sampler_asserts_on_missing_keys(missing):
    from gaia_seg_amd.apis import sandwich_train_sampler
    with pytest.raises(AssertionError):
        sandwich_train_sampler(_cfg(**{missing: None}))


def test_inplace_distill_config_expands_to_the_sandwich():
    from gaia_seg_amd.apis import sandwich_train_sampler
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.model_space import build_model_sampler
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_inplace_distill.py"))
    assert cfg.use_distillation and cfg.sample_subnet_num == 3
    assert dict(cfg.distill_cfg) == dict(T=2.0, distillation_weight=0.5, interpolation=False)
    assert cfg.model.decode_head.type == "DynamicPSPHead"
    assert cfg.model.auxiliary_head.type == "DynamicFCNHead"
    s = build_model_sampler(sandwich_train_sampler(cfg))
    s.seed(3)
    members = s.candidates()
    assert [m.get("name") for m in members] == ["MAX", "MIN", None, None, None]
    bb = cfg.model.backbone
    arch = fold_dict(members[0])["arch"]["backbone"]
    assert arch == {"stem": {"width": bb.stem_width},
                    "body": {"width": list(bb.body_width), "depth": list(bb.body_depth)}}


def _model(head, aux=True):
    from util_models import model_cfg
    from gaia_seg_amd.models import build_segmentor
    return build_segmentor(model_cfg(head, aux=aux))


def test_head_combinations_for_the_sandwich():
    from util_models import fcn_head, psp_head, uper_head
    from gaia_seg_amd.core.runner import check_sandwich_model
    check_sandwich_model(_model(psp_head(), aux=True))
    check_sandwich_model(_model(psp_head(), aux=False))
    with pytest.raises(ValueError, match="aux_teacher_logits"):
        check_sandwich_model(_model(fcn_head(), aux=True))
    with pytest.raises(ValueError, match="no distillation branch"):
        check_sandwich_model(_model(uper_head(), aux=True))


def test_uper_head_refuses_teacher_logits():
    from util_models import uper_head
    m = _model(uper_head(), aux=False)
    with pytest.raises(NotImplementedError, match="no in-place distillation branch"):
        m.decode_head.forward_train([], None, None, None, teacher_logits=torch.zeros(1))


def test_sandwich_hook_validates_its_inputs():
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import SandwichHook
    anchor = build_model_sampler(dict(type="anchor", anchors=[{"name": "MAX"}]))
    with pytest.raises(TypeError):
        SandwichHook(anchor)
    concat = build_model_sampler(dict(type="concat", model_samplers=[dict(type="anchor", anchors=[{}])]))
    with pytest.raises(KeyError):
        SandwichHook(concat, dict(temperature=2))
    assert SandwichHook(concat, dict(T=4)).kd_cfg == dict(T=4, distillation_weight=0.5, interpolation=False)


def test_ranges_union():
    from gaia_seg_amd.core.runner import _ranges_union
    assert _ranges_union([(0, 64), (128, 256)], [(64, 128), (512, 576)]) == [(0, 256), (512, 576)]
    assert _ranges_union([], [(0, 64)]) == [(0, 64)]


def _desc(**kw):
    d = lib.KdDesc(N=2, h=4, w=6, Cls=19, H=32, W=48, s_sn=4 * 6 * 20, s_sh=6 * 20, s_sw=20, s_sc=1,
                   t_sn=4 * 6 * 20, t_sh=6 * 20, t_sw=20, t_sc=1, T=2.0, align_corners=0,
                   interpolation=1, reserved=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_kd_c_abi_argument_validation_needs_no_gpu():
    L = lib.load()
    assert ctypes.sizeof(lib.KdDesc) == 6 * 4 + 8 * 8 + 4 * 4
    d = _desc()
    assert L.gs_kd_workspace_bytes(ctypes.byref(d)) > 0
    assert L.gs_kd_backward_workspace_bytes(ctypes.byref(d), 20) == 2 * 5 * 7 * 4 * 20 * 4
    assert L.gs_kd_backward_workspace_bytes(ctypes.byref(d), 18) == 0          # ld < Cls
    assert L.gs_kd_backward_workspace_bytes(ctypes.byref(_desc(interpolation=0, H=4, W=6)), 20) == 0
    for bad in (dict(N=0), dict(Cls=0), dict(H=0), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")),
                dict(T=float("nan")), dict(interpolation=2), dict(interpolation=0)):   # no interp: H, W must be h, w
        bd = _desc(**bad)
        assert L.gs_kd_workspace_bytes(ctypes.byref(bd)) == 0, bad
        assert L.gs_kd_forward(ctypes.byref(bd), 16, 16, None, None, 1.0, 16, 16, 1 << 20, None) == -1, bad
        assert L.gs_kd_backward(ctypes.byref(bd), 16, 16, 16, 16, 1.0, 16, 20, None, 0, None) == -1, bad
    assert L.gs_kd_forward(None, 16, 16, None, None, 1.0, 16, 16, 1 << 20, None) == -4
    assert L.gs_kd_forward(ctypes.byref(d), None, 16, None, None, 1.0, 16, 16, 1 << 20, None) == -4
    assert L.gs_kd_forward(ctypes.byref(d), 16, 16, None, None, 1.0, None, 16, 1 << 20, None) == -4
    assert L.gs_kd_forward(ctypes.byref(d), 16, 16, None, None, 1.0, 16, None, 1 << 20, None) == -4
    assert L.gs_kd_forward(ctypes.byref(d), 16, 16, None, None, 1.0, 16, 16, 8, None) == -3
    assert L.gs_kd_forward(ctypes.byref(d), 16, 16, None, None, 1.0, 16, 20, 1 << 20, None) == -2
    assert L.gs_kd_backward(ctypes.byref(d), 16, 16, None, 16, 1.0, 16, 20, None, 0, None) == -4
    assert L.gs_kd_backward(ctypes.byref(d), 16, 16, 16, 16, 1.0, 16, 18, None, 0, None) == -1


def test_grad_accumulate_argument_validation_needs_no_gpu():
    L = lib.load()
    assert L.gs_grad_accumulate(None, 16, 4, None) == -4
    assert L.gs_grad_accumulate(16, None, 4, None) == -4
    assert L.gs_grad_accumulate(16, 32, -1, None) == -1
    assert L.gs_grad_accumulate(16, 16, 4, None) == -1
    assert L.gs_grad_accumulate(16, 32, 0, None) == 0        # nothing to do: no launch
