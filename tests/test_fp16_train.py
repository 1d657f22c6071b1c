"""fp16 training without a GPU: the training-precision switch's dispatch (gs_debug_query_conv_launch:
host arithmetic only), the Fp16OptimizerHook config forms, and the loss scaler's state and rules
(mmcv's LossScaler)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _query(L, lib, d, op):
    q = lib.DebugLaunch()
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q)) == 0
    return (q.kloop, q.bm, q.bn, q.splits, q.ksteps_per_split)


def test_train_precision_dispatch_without_gpu():
    from gaia_seg_amd.hip import lib
    from test_dgrad_x3_gpu import X3_CASES
    L = lib.load()
    assert L.gs_get_train_precision() == 0
    assert L.gs_set_train_precision(2) == -1 and L.gs_set_train_precision(-1) == -1
    descs = []
    for case in X3_CASES:
        n, h, w, ci, co, k, dil, ci_max, co_ld, ldx, ldy = case[:11]
        descs.append((case, lib.conv_desc(n, h, w, ci, co, k, dil=dil, ci_max=ci_max, co_ld=co_ld,
                                          ldx=ldx, ldy=ldy)))
    ops_ = (lib.OP_FORWARD, lib.OP_DGRAD, lib.OP_WGRAD)
    for case, d in descs:
        if case[-1]:
            assert L.gs_debug_force_plan(*case[-1]) == 0
        try:
            before = {op: _query(L, lib, d, op) for op in ops_}
            assert L.gs_set_train_precision(1) == 0
            try:
                assert L.gs_get_train_precision() == 1
                assert L.gs_get_forward_precision() == 0      # the inference switch is untouched
                f16 = {op: _query(L, lib, d, op) for op in ops_}
            finally:
                assert L.gs_set_train_precision(0) == 0
            after = {op: _query(L, lib, d, op) for op in ops_}
        finally:
            L.gs_debug_force_plan(0, 0, 0)
        assert after == before, case                       # switch at 0 == never set
        assert f16[lib.OP_DGRAD][0] == lib.KLOOP_F16, (case, f16[lib.OP_DGRAD])
        assert f16[lib.OP_DGRAD][1] == 64 and f16[lib.OP_DGRAD][2] in (64, 48)
        assert f16[lib.OP_DGRAD][3] == before[lib.OP_DGRAD][3]   # split-K factor unchanged
        assert f16[lib.OP_WGRAD] == before[lib.OP_WGRAD]         # weight gradients stay fp32
        assert f16[lib.OP_WGRAD][0] != lib.KLOOP_F16
        assert before[lib.OP_DGRAD][0] != lib.KLOOP_F16
    assert L.gs_get_train_precision() == 0 and L.gs_get_forward_precision() == 0


def test_train_precision_narrows_80_and_32_column_plans_without_gpu():
    """A data gradient whose plan has 80 (32) columns gets 64 (48) on the f16 loop, same splits and
    workspace; the weight gradient of the same conv is untouched."""
    from gaia_seg_amd.hip import lib
    L = lib.load()
    seen = set()
    for (n, h, w, ci, co) in [(2, 64, 128, 80, 80), (2, 32, 64, 160, 160), (2, 128, 256, 32, 32),
                              (2, 64, 128, 320, 80), (2, 16, 32, 640, 160), (2, 64, 128, 96, 32)]:
        d = lib.ConvDesc(N=n, H=h, W=w, Ci=ci, Co=co, Ci_max=ci, Co_ld=co, KH=3, KW=3, stride=1, pad=1,
                         dil=1, Ho=h, Wo=w, x_sn=h * w * ci, x_sh=w * ci, x_sw=ci, x_sc=1, ldy=co,
                         ld_add=0, role=0, reserved=0, in_affine=None)
        b = _query(L, lib, d, lib.OP_DGRAD)
        ws = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        assert L.gs_set_train_precision(1) == 0
        try:
            q = _query(L, lib, d, lib.OP_DGRAD)
            ws16 = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        finally:
            L.gs_set_train_precision(0)
        assert ws16 == ws
        if b[1] == 64:
            assert q[0] == lib.KLOOP_F16 and q[3] == b[3], (b, q)
            assert q[2] == {80: 64, 32: 48}.get(b[2], b[2]), (b, q)
            seen.add(b[2])
    assert seen & {80, 32}, seen      # at least one plan was narrowed


def test_train_precision_context_manager_restores_without_gpu():
    from gaia_seg_amd.hip import lib, ops
    L = lib.load()
    with ops.train_precision("fp16"):
        assert L.gs_get_train_precision() == 1 and L.gs_get_forward_precision() == 0
        assert ops.FORWARD_PRECISION == lib.PRECISION_FP32
    assert L.gs_get_train_precision() == 0
    with pytest.raises(KeyError):
        with ops.train_precision("fp16"):
            raise KeyError("boom")
    assert L.gs_get_train_precision() == 0
    with pytest.raises(ValueError):
        ops.train_precision("bf16")


def test_fp16_optimizer_config_forms():
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, Fp16ArenaOptimizerHook
    h = optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=512.))
    assert isinstance(h, Fp16ArenaOptimizerHook)
    assert h.loss_scaler.state_dict() == dict(cur_scale=512., cur_iter=0, mode="static",
                                              last_overflow_iter=-1, scale_factor=2.,
                                              scale_window=1000)
    assert optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=64)).loss_scaler.loss_scale == 64.
    assert optimizer_hook(dict(type="Fp16OptimizerHook")).loss_scaler.loss_scale == 512.   # mmcv's default
    for plain in (None, {}, dict(), dict(type="OptimizerHook"), dict(grad_clip=None)):
        h = optimizer_hook(plain)
        assert type(h) is ArenaOptimizerHook, plain
    with pytest.raises(NotImplementedError, match="grad_clip"):
        optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=512., grad_clip=dict(max_norm=35)))
    with pytest.raises(NotImplementedError, match="grad_clip"):
        optimizer_hook(dict(grad_clip=dict(max_norm=35)))
    for dyn in ("dynamic", dict(init_scale=2. ** 32, scale_factor=2., scale_window=1000)):
        with pytest.raises(NotImplementedError, match="dynamic loss scaling"):
            optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=dyn))
    for bad in (0, -1., float("nan"), float("inf"), "static", True, [512]):
        with pytest.raises(ValueError):
            optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=bad))


def test_fp16_config_and_distillation_refused():
    from gaia_seg_amd.apis.train import optimizer_hook, train_segmentor
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_fp16.py"))
    assert dict(cfg.optimizer_config) == dict(type="Fp16OptimizerHook", loss_scale=512.)
    assert optimizer_hook(cfg.optimizer_config).loss_scaler.loss_scale == 512.
    # a top-level fp16 key alone keeps meaning fp16 evaluation: the optimizer stays fp32
    plain = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2.py"))
    assert type(optimizer_hook(plain.get("optimizer_config"))).__name__ == "ArenaOptimizerHook"
    # use_distillation + fp16: refused at set-up, before any model is built or moved
    dist_cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet",
                                            "pspnet_ar50to101v2_inplace_distill.py"))
    dist_cfg.optimizer_config = dict(type="Fp16OptimizerHook", loss_scale=512.)

    class _Refuse:
        def to(self, *a, **k):
            raise AssertionError("set-up went past the fp16 + distillation check")
    with pytest.raises(ValueError, match="use_distillation"):
        train_segmentor(_Refuse(), None, None, None, dist_cfg)


def test_loss_scaler_rules():
    """mmcv's LossScaler, step by step (the state a checkpoint stores under meta.fp16.loss_scaler)."""
    from gaia_seg_amd.core.fp16_utils import LossScaler
    s = LossScaler(init_scale=2. ** 20, mode="dynamic", scale_factor=2., scale_window=2)
    trace = []
    for overflow in (True, True, False, False, False, True, False, False):
        s.update_scale(overflow)
        trace.append((s.cur_scale, s.cur_iter, s.last_overflow_iter))
    assert trace == [(2. ** 19, 1, 0), (2. ** 18, 2, 1), (2. ** 18, 3, 1), (2. ** 19, 4, 1),
                     (2. ** 19, 5, 1), (2. ** 18, 6, 5), (2. ** 18, 7, 5), (2. ** 19, 8, 5)]
    low = LossScaler(init_scale=1., mode="dynamic")
    low.update_scale(True)
    assert low.cur_scale == 1                          # never below 1
    st = LossScaler(init_scale=512., mode="static")
    for ov in (True, False):
        st.update_scale(ov)
    assert st.state_dict() == dict(cur_scale=512., cur_iter=0, mode="static", last_overflow_iter=-1,
                                   scale_factor=2., scale_window=1000)
    r = LossScaler()
    r.load_state_dict(s.state_dict())
    assert r.state_dict() == s.state_dict()
    with pytest.raises(ValueError):
        LossScaler(mode="half")
