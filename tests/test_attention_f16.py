"""The fp16 attention switch without a GPU: the host-side argument checks of the gs_attention_*_f16 entries,
wrap_fp16_model(attention=...), the type check of ``fp16.attention``, what apis.train.optimizer_hook makes
of the key, the finetune snapshot, the step-graph key and the new config."""
import copy
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import util_vit as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
OK_PTR, ODD_PTR = 1 << 20, (1 << 20) + 4      # never read: every call below is refused before a launch
NEW = ("gs_attention_forward_f16", "gs_attention_relpos_forward_f16", "gs_attention_workspace_bytes_f16",
       "gs_attention_backward_f16")


def test_header_binding_and_exports_agree_with_the_new_symbols(hip_lib):
    import test_c_abi
    from gaia_seg_amd.hip import lib
    test_c_abi.test_header_and_binding_agree()
    test_c_abi.test_library_exports_every_symbol()
    for name in NEW:
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)
        assert lib.PROTOTYPES[name] == lib.PROTOTYPES[name[:-len("_f16")]], "the twins share their signatures"


def test_f16_entries_check_their_arguments_before_any_launch(hip_lib):
    from gaia_seg_amd.hip import lib
    L = hip_lib

    def desc(n=7, heads=2, **kw):
        d = lib.attention_desc(1, n, heads)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    def ref(d):
        return ctypes.byref(d) if d is not None else None

    def fwd(d, q=OK_PTR, o=OK_PTR, lse=OK_PTR):
        return L.gs_attention_forward_f16(ref(d), q, OK_PTR, OK_PTR, o, lse, None)

    def rel(d, q=OK_PTR, table=OK_PTR, ld_table=2, wh=2, ww=3, o=OK_PTR):
        return L.gs_attention_relpos_forward_f16(ref(d), q, OK_PTR, OK_PTR, table, ld_table, wh, ww, o, OK_PTR, None)

    def bwd(d, dq=OK_PTR, ws=OK_PTR, ws_bytes=1 << 20, do=OK_PTR):
        return L.gs_attention_backward_f16(ref(d), OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, do, dq, OK_PTR, OK_PTR,
                                           0, ws, ws_bytes, None)

    def need(d):
        return L.gs_attention_workspace_bytes_f16(ref(d))

    assert fwd(None) == rel(None) == bwd(None) == GS_E_NULL and need(None) == 0
    assert fwd(desc(), q=None) == fwd(desc(), o=None) == fwd(desc(), lse=None) == GS_E_NULL
    assert rel(desc(), table=None) == rel(desc(), q=None) == GS_E_NULL
    assert bwd(desc(), dq=None) == bwd(desc(), ws=None) == bwd(desc(), do=None) == GS_E_NULL
    for bad in (desc(n=0), desc(heads=0), desc(scale=0.0), desc(ldq=124), desc(ldo=64), desc(lddv=124), desc(B=0)):
        assert fwd(bad) == rel(bad) == bwd(bad) == GS_E_BADARG and need(bad) == 0
    for bad in (desc(ldk=130), desc(lddq=129)):
        assert fwd(bad) == rel(bad) == bwd(bad) == GS_E_ALIGN and need(bad) == 0
    assert fwd(desc(), q=ODD_PTR) == fwd(desc(), o=ODD_PTR) == GS_E_ALIGN
    assert rel(desc(), q=ODD_PTR) == rel(desc(), table=OK_PTR + 2) == GS_E_ALIGN
    assert bwd(desc(), dq=ODD_PTR) == bwd(desc(), ws=ODD_PTR) == GS_E_ALIGN
    assert rel(desc(n=8)) == rel(desc(), wh=0) == rel(desc(), ld_table=1) == GS_E_BADARG
    assert rel(desc(n=64 * 64 + 1), wh=64, ww=64) == GS_E_BADARG       # the table would not fit in LDS
    # delta[B][heads][N] and one maximum per (batch, head, 128 tokens), rounded up to 16 bytes
    for n, heads in ((7, 2), (128, 1), (129, 3), (2049, 12)):
        want = 4 * heads * (n + (n + 127) // 128)
        assert need(desc(n=n, heads=heads)) == (want + 15) // 16 * 16
        assert need(desc(n=n, heads=heads)) > L.gs_attention_workspace_bytes(ref(desc(n=n, heads=heads))) - 16
    d = desc(n=129, heads=3)
    assert bwd(d, ws_bytes=need(d) - 1) == bwd(d, ws_bytes=0) == GS_E_WORKSPACE


def tiny_segmentor():
    from gaia_seg_amd.models import build_segmentor
    return build_segmentor(copy.deepcopy(U.tiny_model_cfg()))


def flags(model):
    return [m.fp16_attention for m in model.modules() if hasattr(m, "fp16_attention")]


def test_wrap_fp16_model_attention():
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    from gaia_seg_amd.models.backbones.elastic_transformer import ElasticMHA
    model = tiny_segmentor()
    n_attn = sum(isinstance(m, ElasticMHA) for m in model.modules())
    assert n_attn == 4 and flags(model) == [False] * (n_attn + 1) and model.backbone.fp16_attention is False
    assert wrap_fp16_model(model) is model
    assert model.fp16_enabled is True and not any(flags(model)), "without attention=True nothing changes"
    wrap_fp16_model(model, attention=True)
    assert all(flags(model)) and model.backbone.fp16_attention is True
    model.backbone.fp16_attention = False       # the backbone's attribute is the switch of its layers
    assert not any(flags(model))
    # attention=None (the default): the key of the config the model was built from, if there is one
    for top, want in ((dict(fp16=dict(attention=True)), True), (dict(fp16=dict(loss_scale=512.)), False),
                      (dict(), False)):
        model.top_cfg = top
        model.backbone.fp16_attention = False
        wrap_fp16_model(model)
        assert flags(model) == [want] * 5, top
        wrap_fp16_model(model, attention=False)     # an explicit value wins, and False sets nothing
        assert flags(model) == [want] * 5
    model.top_cfg = dict(fp16=dict(attention=1))
    with pytest.raises(ValueError, match="fp16.attention"):
        wrap_fp16_model(model)
    # a model without such a module: the key would do nothing, so it is an error
    from util_models import fcn_head, make_pair, model_cfg
    cnn = make_pair(model_cfg(fcn_head(), aux=False))[0]
    wrap_fp16_model(cnn)
    with pytest.raises(ValueError, match="fp16_attention"):
        wrap_fp16_model(cnn, attention=True)


def test_beit_has_the_flag():
    from gaia_seg_amd.models import build_backbone
    from util_beit import tiny_cfg
    m = build_backbone(tiny_cfg("p16-block-tables"))
    assert m.fp16_attention is False and flags(m) == [False] * (len(m.blocks) + 1)
    m.fp16_attention = True
    assert all(flags(m))


@pytest.mark.parametrize("bad", [1, 0, "yes", None, [True]])
def test_fp16_attention_must_be_a_bool(bad):
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.fp16_utils import check_fp16_cfg
    with pytest.raises(ValueError, match="fp16.attention"):
        check_fp16_cfg(dict(attention=bad))
    with pytest.raises(ValueError, match="fp16.attention"):     # with and without the fp16 hook
        optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=512.), dict(attention=bad))
    with pytest.raises(ValueError, match="fp16.attention"):
        optimizer_hook(None, dict(attention=bad))


def test_optimizer_hook_with_and_without_the_key():
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.fp16_utils import check_fp16_cfg
    assert check_fp16_cfg(None) is False and check_fp16_cfg(dict()) is False
    assert check_fp16_cfg(dict(loss_scale=512.)) is False and check_fp16_cfg(dict(attention=True)) is True
    oc = dict(type="Fp16OptimizerHook", loss_scale=512.)
    assert optimizer_hook(oc).attention is False and optimizer_hook(oc, dict()).attention is False
    assert optimizer_hook(oc, dict(attention=False)).attention is False
    hook = optimizer_hook(oc, dict(attention=True))
    assert hook.attention is True and hook.loss_scaler.loss_scale == 512.
    # without the fp16 hook the key keeps cfg.fp16's meaning (evaluation only): the fp32 hook, untouched
    plain = optimizer_hook(None, dict(attention=True))
    assert type(plain).__name__ == "ArenaOptimizerHook" and not hasattr(plain, "attention")
    # before_run wraps the model
    for attention in (False, True):
        model = tiny_segmentor()
        runner = SimpleNamespace(hooks=[], model=model, meta=None)
        optimizer_hook(oc, dict(attention=attention)).before_run(runner)
        assert model.fp16_enabled is True and runner.train_precision == "fp16" and runner.loss_scale == 512.
        assert flags(model) == [attention] * 5


def test_finetune_snapshot_restores_the_flag():
    from gaia_seg_amd.apis.finetune import SupernetSnapshot
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    model = tiny_segmentor()
    arena = SimpleNamespace(flat_param=torch.zeros(4), flat_grad=torch.zeros(4), flat_acc=None,
                            reset_optimizer_state=lambda: None, grads_clean=False)
    snap = SupernetSnapshot(model, arena)
    wrap_fp16_model(model, attention=True)       # what a run's fp16 hook does
    assert all(flags(model)) and model.fp16_enabled
    snap.restore()
    assert not any(flags(model)) and model.fp16_enabled is False and model.backbone.fp16_attention is False


def test_step_graph_key_carries_the_flag():
    from gaia_seg_amd.core.runner import IterBasedRunner
    model = tiny_segmentor()
    stub = SimpleNamespace(graphs_enabled=True, graphs_paused=False, arch_key=("sub",), model=model,
                           arena=SimpleNamespace(groups=None), train_precision="fp16", loss_scale=512.)
    off = IterBasedRunner._graph_key(stub, {})
    assert off is not None and IterBasedRunner._graph_key(stub, {}) == off
    model.backbone.fp16_attention = True
    on = IterBasedRunner._graph_key(stub, {})
    assert on is not None and on != off
    model.backbone.fp16_attention = False
    assert IterBasedRunner._graph_key(stub, {}) == off


def test_the_fp16_config_loads():
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.optimizer import check_optimizer_cfg
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit_adamw_fp16.py"))
    base = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "upernet_elastic_vit_adamw.py"))
    assert dict(cfg.fp16) == dict(attention=True)
    assert dict(cfg.optimizer_config) == dict(type="Fp16OptimizerHook", loss_scale=512.)
    assert check_optimizer_cfg(cfg.optimizer) == check_optimizer_cfg(base.optimizer)
    assert dict(cfg.lr_config) == dict(base.lr_config) and cfg.model == base.model
    assert base.get("fp16") is None
    hook = optimizer_hook(cfg.get("optimizer_config"), cfg.get("fp16"))
    assert type(hook).__name__ == "Fp16ArenaOptimizerHook" and hook.attention is True
    # evaluation (tools/test_supernet.py: wrap_fp16_model(model) when cfg.fp16 is set) finds the key through
    # the model's own config
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    from gaia_seg_amd.models import build_segmentor
    for c, want in ((cfg, True), (base, False)):
        model = build_segmentor(c.model)
        wrap_fp16_model(model)
        assert model.fp16_enabled is True and model.backbone.fp16_attention is want
