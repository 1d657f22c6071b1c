"""DynamicDistiller on the MI355X: the two loss operators (csrc/distill.hip gs_distill_*, gs_pairwise_*)
against the fp64 values the reference's own methods produced (tests/golden/ref_distiller.npz), their
C-ABI contracts, one model-level train step against oracle student + oracle teacher + the restatement
of tests/util_distiller.py under the criteria of tests/parity.py, and the runner / finetune / CLI
plumbing around the unregistered teacher.

Bounds.  Loss within 1e-5 relative and gradient within 1e-5 of the largest reference gradient (max
norm): the bar tests/test_inplace_distill_gpu.py sets for gs_kd_*.  For the pairwise operator the bound
is the larger of that and 4x the error of the reference's own fp32 CPU run against its fp64 run on the
same inputs (stored in the fixture; factor 2 for another summation order erring the other way, factor
2 of headroom)."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import util_distiller as U  # noqa: E402
from test_distiller import distiller_cfg, teacher_cfg, write_teacher  # noqa: E402
from util_models import ARCHS, arch_meta, make_batch, model_cfg, psp_head, randomize  # noqa: E402

PROFILE = os.environ.get("GS_DISTILLER_ERRORS")   # path: one JSON line of observed errors per case


def _note(**rec):
    print("[distiller] " + json.dumps(rec))
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def fx():
    return np.load(U.FIXTURE)


# ---- gs_distill_* ------------------------------------------------------------------------------
def _padded(x, ld):
    """[n, c, h, w] values of ``x`` as a view of a padded NHWC buffer (pad columns hold garbage)."""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), 3.25)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.cuda().permute(0, 3, 1, 2)[:, :c]


@pytest.mark.parametrize("tag", list(U.DISTILL_CASES))
def test_distill_op_matches_the_reference_fp64(fx, tag):
    from gaia_seg_amd.models.losses.distill_loss import teacher_distill_loss
    n, c, hs, ht, hw, align, T, wgt = U.DISTILL_CASES[tag]
    s = _padded(torch.from_numpy(fx["kd_%s_s" % tag]), 20).detach().requires_grad_(True)
    t = _padded(torch.from_numpy(fx["kd_%s_t" % tag]), 24)
    loss = teacher_distill_loss(s, t, hw, T=T, weight=wgt, align_corners=align)
    (loss * 1.0).backward()
    ref_l, ref_g = float(fx["kd_%s_loss64" % tag]), torch.from_numpy(fx["kd_%s_grad64" % tag])
    e_l = abs(float(loss) - ref_l) / abs(ref_l)
    e_g = float((s.grad.double().cpu() - ref_g).abs().max() / ref_g.abs().max())
    _note(op="distill", case=tag, loss_relerr=e_l, grad_relerr=e_g)
    assert e_l <= 1e-5, (float(loss), ref_l)
    assert e_g <= 1e-5, e_g
    assert t.grad is None


def _kd_direct(fx, tag, entry, workspace=True):
    """(loss, dense gradient incl. pad columns) through the C-ABI, by gs_distill_* or gs_kd_*."""
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import distill_desc, kd_desc
    L = lib.load()
    n, c, hs, ht, hw, align, T, wgt = U.DISTILL_CASES[tag]
    s = _padded(torch.from_numpy(fx["kd_%s_s" % tag]), 20)
    t = _padded(torch.from_numpy(fx["kd_%s_t" % tag]), 24)
    if entry == "distill":
        d = distill_desc(s, t, hw, T, align)
        fwd, bwd, wsf, wsb = (L.gs_distill_forward, L.gs_distill_backward, L.gs_distill_workspace_bytes,
                              L.gs_distill_backward_workspace_bytes)
    else:
        d = kd_desc(s, t, hw, T, align, True)
        fwd, bwd, wsf, wsb = (L.gs_kd_forward, L.gs_kd_backward, L.gs_kd_workspace_bytes,
                              L.gs_kd_backward_workspace_bytes)
    ld = 20
    lse_s = torch.empty(n, hw[0], hw[1], device="cuda")
    lse_t = torch.empty_like(lse_s)
    out = torch.empty(1, device="cuda")
    need = wsb(ctypes.byref(d), ld)
    assert need > 0
    ws = torch.empty(max(wsf(ctypes.byref(d)), need) // 4 + 4, device="cuda")
    assert fwd(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(), 0.25,
               out.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) == 0
    buf = torch.full((n, hs[0], hs[1], ld), 7.0, device="cuda")
    assert bwd(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(), 0.25,
               buf.data_ptr(), ld, ws.data_ptr() if workspace else None,
               ws.numel() * 4 if workspace else 0, None) == 0
    torch.cuda.synchronize()
    return out.clone(), buf, lse_s, lse_t


@pytest.mark.parametrize("tag", ["e", "f"])
def test_equal_resolution_distill_is_bitwise_gs_kd(fx, tag):
    for workspace in (True, False):
        a = _kd_direct(fx, tag, "distill", workspace)
        b = _kd_direct(fx, tag, "kd", workspace)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_distill_gather_form_reproducibility_and_pad(fx, tag):
    c = U.DISTILL_CASES[tag][1]
    l1, g1, _, _ = _kd_direct(fx, tag, "distill")
    l2, g2, _, _ = _kd_direct(fx, tag, "distill")
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert (g1[..., c:] == 0).all()
    _, gg, _, _ = _kd_direct(fx, tag, "distill", workspace=False)
    err = float((g1[..., :c] - gg[..., :c]).abs().max() / g1[..., :c].abs().max())
    assert err <= 1e-5, err
    assert (gg[..., c:] == 0).all()


# ---- gs_pairwise_* -----------------------------------------------------------------------------
def _pairwise_case(fx, tag):
    n, cs, ct, h, w, T, wgt, seed, nonc = U.PAIRWISE_CASES[tag]
    win = tuple(int(v) for v in fx["pw_%s_window" % tag])
    s = U.embed_window(torch.from_numpy(fx["pw_%s_s" % tag]), h, w, win, seed + 100, nonc)
    t = U.embed_window(torch.from_numpy(fx["pw_%s_t" % tag]), h, w, win, seed + 200)
    return s, t, win, T, wgt


def _to_cuda_keeping_layout(x):
    """The same strides on the device (a channel slice of a wider channels-last buffer stays one)."""
    n, c, h, w = x.shape
    ld = x.stride(3)
    assert x.stride() == (h * w * ld, 1, w * ld, ld)
    buf = torch.zeros(n, h, w, ld)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.cuda()[..., :c].permute(0, 3, 1, 2)


def _pairwise_errors(s, t, win, T, wgt, ref_l, ref_g_win):
    from gaia_seg_amd.models.losses.distill_loss import pairwise_loss
    y0, y1, x0 = win[:3]
    sc = _to_cuda_keeping_layout(s).detach().requires_grad_(True)
    tc = _to_cuda_keeping_layout(t)
    loss = pairwise_loss(sc, tc, win, T=T, weight=wgt)
    (loss * 1.0).backward()
    g = sc.grad.double().cpu()
    mask = torch.ones(s.shape[2], s.shape[3], dtype=torch.bool)
    mask[y0:y1, x0] = False
    assert (g[:, :, mask] == 0).all() and torch.isfinite(g).all() and tc.grad is None
    e_l = abs(float(loss) - ref_l) / abs(ref_l)
    e_g = float((g[:, :, y0:y1, x0] - ref_g_win).abs().max() / ref_g_win.abs().max())
    return e_l, e_g


@pytest.mark.parametrize("tag", list(U.PAIRWISE_CASES))
def test_pairwise_op_matches_the_reference_fp64(fx, tag):
    s, t, win, T, wgt = _pairwise_case(fx, tag)
    l64, g64 = float(fx["pw_%s_loss64" % tag]), torch.from_numpy(fx["pw_%s_grad64" % tag])
    l32, g32 = float(fx["pw_%s_loss32" % tag]), torch.from_numpy(fx["pw_%s_grad32" % tag]).double()
    ref_el = abs(l32 - l64) / abs(l64)
    ref_eg = float((g32 - g64).abs().max() / g64.abs().max())
    e_l, e_g = _pairwise_errors(s, t, win, T, wgt, l64, g64)
    _note(op="pairwise", case=tag, loss_relerr=e_l, grad_relerr=e_g, ref32_loss_relerr=ref_el,
          ref32_grad_relerr=ref_eg)
    assert e_l <= max(1e-5, 4 * ref_el), (e_l, ref_el)
    assert e_g <= max(1e-5, 4 * ref_eg), (e_g, ref_eg)


def test_pairwise_op_at_the_production_width(fx):
    s, t, win = U.production_inputs()
    T, wgt = U.PRODUCTION[5], U.PRODUCTION[6]
    assert win == tuple(int(v) for v in fx["pw_prod_window"])
    l64, g64 = U.loss_and_grad(U.ref_pairwise_loss, s.double(), t.double(), win, T, wgt)
    assert abs(float(l64) - float(fx["pw_prod_loss64"])) <= 1e-12 * abs(float(l64))   # the same inputs
    ref_el, ref_eg = float(fx["pw_prod_ref32_loss_relerr"]), float(fx["pw_prod_ref32_grad_relerr"])
    y0, y1, x0 = win[:3]
    e_l, e_g = _pairwise_errors(s, t, win, T, wgt, float(l64), g64[:, :, y0:y1, x0])
    _note(op="pairwise", case="production", loss_relerr=e_l, grad_relerr=e_g, ref32_loss_relerr=ref_el,
          ref32_grad_relerr=ref_eg)
    assert e_l <= max(1e-5, 4 * ref_el), (e_l, ref_el)
    assert e_g <= max(1e-5, 4 * ref_eg), (e_g, ref_eg)


def _pairwise_direct(s, t, win, T, ld_extra=4):
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import pairwise_desc
    L = lib.load()
    d = pairwise_desc(s, t, win, T)
    nbytes = L.gs_pairwise_save_bytes(ctypes.byref(d))
    assert nbytes > 0
    save = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.empty(1, device="cuda")
    assert L.gs_pairwise_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), 0.5, out.data_ptr(),
                                 save.data_ptr(), save.numel() * 8, None) == 0
    n, c, h, w = s.shape
    ld = (c + 3) // 4 * 4 + ld_extra
    buf = torch.full((n, h, w, ld), 7.0, device="cuda")
    assert L.gs_pairwise_backward(ctypes.byref(d), s.data_ptr(), save.data_ptr(), save.numel() * 8, 0.5,
                                  buf.data_ptr(), ld, None) == 0
    torch.cuda.synchronize()
    return out.clone(), buf


@pytest.mark.parametrize("tag", ["b", "c"])
def test_pairwise_launches_are_bitwise_reproducible_and_zero_the_pad(fx, tag):
    s, t, win, T, _ = _pairwise_case(fx, tag)
    s, t = _to_cuda_keeping_layout(s), _to_cuda_keeping_layout(t)
    l1, g1 = _pairwise_direct(s, t, win, T)
    l2, g2 = _pairwise_direct(s, t, win, T)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert (g1[..., s.shape[1]:] == 0).all() and g1[..., :s.shape[1]].any()


def test_pairwise_scalar_layout_agrees_with_the_float4_layout(fx):
    """A plain NCHW-contiguous map (channel stride H*W) takes the scalar loads."""
    s, t, win, T, _ = _pairwise_case(fx, "a")
    sv, tv = _to_cuda_keeping_layout(s), _to_cuda_keeping_layout(t)
    l1, g1 = _pairwise_direct(sv, tv, win, T)
    l2, g2 = _pairwise_direct(sv.contiguous(), tv.contiguous(), win, T)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_pairwise_window_above_the_cap_is_refused():
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import pairwise_desc, pairwise_loss
    L = lib.load()
    p = lib.PAIRWISE_MAX_P
    s = torch.rand(1, p + 1, 1, 8, device="cuda").permute(0, 3, 1, 2)     # [1, 8, P + 1, 1]
    d = pairwise_desc(s, s, (0, p + 1, 0, 1), 1.0)
    out = torch.empty(1, device="cuda")
    save = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert L.gs_pairwise_forward(ctypes.byref(d), s.data_ptr(), s.data_ptr(), 1.0, out.data_ptr(),
                                 save.data_ptr(), save.numel() * 8, None) == -1
    with pytest.raises(lib.HipLibraryError):
        pairwise_loss(s.detach().requires_grad_(True), s, (0, p + 1, 0, 1, p + 1, 1))
    d = pairwise_desc(s, s, (0, p, 0, 1), 1.0)                             # exactly the cap runs
    assert L.gs_pairwise_forward(ctypes.byref(d), s.data_ptr(), s.data_ptr(), 1.0, out.data_ptr(),
                                 save.data_ptr(), save.numel() * 8, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_zero_vector_pixels_give_finite_gradients(fx):
    from gaia_seg_amd.models.losses.distill_loss import pairwise_loss
    s, t, win, T, wgt = _pairwise_case(fx, "zero")
    y0, x0 = win[0], win[2]
    assert (s[0, :, y0 + 1, x0] == 0).all() and (t[1, :, y0 + 2, x0] == 0).all()
    sc = _to_cuda_keeping_layout(s).detach().requires_grad_(True)
    loss = pairwise_loss(sc, _to_cuda_keeping_layout(t), win, T=T, weight=wgt)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(sc.grad).all()
    g64 = torch.from_numpy(fx["pw_zero_grad64"])
    g32 = torch.from_numpy(fx["pw_zero_grad32"]).double()
    # The zero-vector pixels' gradients (g / 1e-12) dwarf the others in the max norm of the whole map,
    # so the pixels that are not zero vectors are held to the module's bound one by one, each against
    # its own largest reference gradient.
    got = sc.grad.double().cpu()[:, :, win[0]:win[1], x0]
    for n_, p_ in ((0, 0), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)):
        ref = g64[n_, :, p_]
        scale = float(ref.abs().max())
        ref_e = float((g32[n_, :, p_] - ref).abs().max()) / scale
        e = float((got[n_, :, p_] - ref).abs().max()) / scale
        _note(op="pairwise", case="zero/pixel(%d,%d)" % (n_, p_), grad_relerr=e, ref32_grad_relerr=ref_e)
        assert e <= max(1e-5, 4 * ref_e), (n_, p_, e, ref_e)


# ---- the segmentor -------------------------------------------------------------------------------
class ODistiller(torch.nn.Module):
    """Oracle of the distiller: oracle student + oracle teacher (eval mode, its own ReLU branches,
    outside registration like the product's) + the restatement of both losses."""

    def __init__(self, student, teacher, window, align_corners=False):
        super().__init__()
        self.backbone, self.decode_head = student.backbone, student.decode_head
        self.auxiliary_head = student.auxiliary_head
        self.__dict__["teacher"] = teacher.eval()
        for m in teacher.modules():
            if hasattr(m, "_gs_name"):
                m._gs_name = None      # unkeyed: plain torch.relu
        self.window, self.align_corners = window, align_corners
        self.parse_losses = student.parse_losses

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        self.teacher._apply(fn, *a, **k)
        return self

    def forward_train(self, img, gt):
        # The supplied branch pattern (ReLU masks and the max-pool taps, whose key "backbone.maxpool"
        # is the same in every oracle backbone) describes the student alone, as on the product side
        # (DynamicDistiller.prepare_distill_feature): the teacher runs outside the ReluMasks context.
        from oracle import ops as O
        ctx, O._RELU_CTX = O._RELU_CTX, None
        try:
            with torch.no_grad():
                xt = self.teacher.backbone(img)
                t = self.teacher.decode_head(xt)
        finally:
            O._RELU_CTX = ctx
        x = self.backbone(img)
        s = self.decode_head(x)
        losses = dict(self.decode_head.losses(s, gt))
        losses["distill_loss_seg"] = U.ref_distill_loss(s, t, img.shape[2:], 1.0, 1.0, self.align_corners)
        losses["pairwise_loss_seg"] = U.ref_pairwise_loss(x[-1], xt[-1], self.window, 1.0, 1.0)
        losses.update({"aux." + k: v for k, v in self.auxiliary_head.forward_train(x, gt).items()})
        return losses


@pytest.mark.parametrize("student_os8", [False, True], ids=["os32_under_os8", "os8_under_os8"])
def test_distiller_train_step_against_the_oracle(tmp_path, student_os8):
    import parity
    from oracle.model import OEncoderDecoder
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    tcfg = teacher_cfg(os8=True)
    t_prod = write_teacher(ck, tcfg)
    prod = build_segmentor(distiller_cfg(str(ck), teacher=tcfg, student_os8=student_os8))
    randomize(prod, 0)
    scfg = model_cfg(psp_head(), aux=True, os8=student_os8)
    o_student = OEncoderDecoder(**{k: v for k, v in copy.deepcopy(scfg).items() if k != "type"})
    o_student.load_state_dict({k: v.detach().clone().contiguous() for k, v in prod.state_dict().items()})
    o_teacher = OEncoderDecoder(**{k: v for k, v in copy.deepcopy(tcfg).items() if k != "type"})
    o_teacher.load_state_dict({k: v.detach().clone().contiguous() for k, v in t_prod.state_dict().items()})
    prod = prod.cuda().train()
    assert next(prod.teacher_segmentor.parameters()).is_cuda      # _apply carried the teacher along
    prod.manipulate_arch(arch_meta("sub"))
    o_student.manipulate_arch(arch_meta("sub"))
    img, gt = make_batch(2, 64, 64, seed=2)
    fh = 8 if student_os8 else 2
    seed = 7
    window = U.window_of(fh, fh, seed)
    orc = ODistiller(o_student, o_teacher, window).train()
    assert not orc.teacher.training
    np.random.seed(seed)
    errs = parity.train_step_parity(prod, orc, img, gt)
    assert errs["loss"] < parity.TOL


def test_distiller_loss_keys_and_teacher_untouched(tmp_path):
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    prod = build_segmentor(distiller_cfg(str(ck), student_os8=True))
    randomize(prod, 0)
    prod = prod.cuda().train()
    img, gt = make_batch(2, 64, 64, seed=2)
    np.random.seed(3)
    out = prod.train_step(dict(img=img.cuda(), img_metas=[{}] * 2, gt_semantic_seg=gt.cuda()), None)
    assert list(out["log_vars"]) == ["loss_seg", "acc_seg", "distill_loss_seg", "pairwise_loss_seg",
                                     "aux.loss_seg", "aux.acc_seg", "loss"]
    lv = out["log_vars"]
    total = ((lv["loss_seg"] + lv["distill_loss_seg"]) + lv["pairwise_loss_seg"]) + lv["aux.loss_seg"]
    assert torch.equal(out["loss"].detach(), total)
    assert float(lv["pairwise_loss_seg"]) > 0 and float(lv["distill_loss_seg"]) > 0
    out["loss"].backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in prod.teacher_segmentor.parameters())
    with pytest.raises(TypeError):     # the sandwich's kwargs have no place in this forward_train
        prod.train_step(dict(img=img.cuda(), img_metas=[{}] * 2, gt_semantic_seg=gt.cuda()), None,
                        return_logits=True)


_SUB = {"name": "SUB", "arch.backbone.stem.width": ARCHS["sub"]["stem"],
        "arch.backbone.body.width": list(ARCHS["sub"]["width"]),
        "arch.backbone.body.depth": list(ARCHS["sub"]["depth"])}


def _runner(model, sandwich=False):
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import (ArenaOptimizerHook, FixedLrUpdaterHook, IterBasedRunner,
                                          ManipulateArchHook)
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments, bucket_bytes=1 << 20),
                             base_lr=0.05, momentum=0.9, weight_decay=5e-4, max_iters=100)
    runner.register_hook(ManipulateArchHook(build_model_sampler(dict(type="anchor", anchors=[_SUB]))))
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    return runner, arena


def _batches(seeds, h=64, w=64):
    out = []
    for s in seeds:
        img, gt = make_batch(2, h, w, seed=s)
        out.append(dict(img=img.cuda(), img_metas=[dict(ori_shape=(h, w, 3), img_shape=(h, w, 3),
                                                        pad_shape=(h, w, 3), flip=False)] * 2,
                        gt_semantic_seg=gt.cuda()))
    return out


def test_flags_off_is_bitwise_the_plain_model():
    from gaia_seg_amd.models import build_segmentor
    a = build_segmentor(distiller_cfg(None, has_distill_loss=False, has_pairwise_loss=False))
    randomize(a, 3)
    b = build_segmentor(model_cfg(psp_head(), aux=True))
    randomize(b, 3)
    ra, aa = _runner(a.cuda().train())
    rb, ab = _runner(b.cuda().train())
    for batch in _batches((1, 2, 3)):
        oa, ob = ra.train_iter(batch), rb.train_iter(batch)
        assert torch.equal(oa["loss"], ob["loss"])
        assert set(oa["log_vars"]) == {"loss_seg", "acc_seg", "aux.loss_seg", "aux.acc_seg", "loss"}
    torch.cuda.synchronize()
    assert torch.equal(aa.flat_param, ab.flat_param) and torch.equal(aa.flat_mom, ab.flat_mom)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sb)


def test_a_distiller_step_is_never_captured(monkeypatch):
    """With step graphs switched on a named anchor is captured when it comes back; a distiller's is not."""
    from gaia_seg_amd.models import build_segmentor
    monkeypatch.setenv("GS_STEP_GRAPH", "1")
    a = build_segmentor(distiller_cfg(None, has_distill_loss=False, has_pairwise_loss=False))
    randomize(a, 3)
    ra, _ = _runner(a.cuda().train())
    assert ra.graphs_enabled
    for batch in _batches((1, 2, 3)):
        ra.train_iter(batch)
        assert ra._graph_key(batch) is None
    torch.cuda.synchronize()
    assert ra.graph_stats == {"captured": 0, "replayed": 0, "eager": 3}


def test_three_distilled_iterations_leave_the_teacher_alone(tmp_path):
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.core.runner import SandwichHook
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    model = build_segmentor(distiller_cfg(str(ck), student_os8=True))
    randomize(model, 3)
    model = model.cuda().train()
    t = model.teacher_segmentor
    before = {k: v.detach().clone() for k, v in t.state_dict().items()}
    runner, arena = _runner(model)
    p0 = arena.flat_param.clone()
    np.random.seed(0)
    for batch in _batches((1, 2, 3)):
        out = runner.train_iter(batch)
        assert torch.isfinite(out["loss"]).item()
    torch.cuda.synchronize()
    assert not torch.equal(p0, arena.flat_param)
    after = t.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert not t.training and all(p.grad is None for p in t.parameters())
    # no arena segment: no teacher tensor lives inside the flat parameter storage
    lo = arena.flat_param.data_ptr()
    hi = lo + arena.flat_param.numel() * 4
    assert all(not (lo <= p.data_ptr() < hi) for p in t.parameters())
    assert set(arena.segments) == {id(p) for p in model.parameters()}
    assert not set(arena.segments) & {id(p) for p in t.parameters()}
    assert set(arena.names.values()) == {k for k, _ in model.named_parameters()}
    save_checkpoint(model, str(tmp_path / "iter_3.pth"), optimizer=arena)
    saved = torch.load(str(tmp_path / "iter_3.pth"), map_location="cpu")
    plain = build_segmentor(model_cfg(psp_head(), aux=True, os8=True))
    assert list(saved["state_dict"]) == list(plain.state_dict())
    # the sandwich does not combine with a fixed teacher
    from gaia_seg_amd.core.model_space import build_model_sampler
    concat = build_model_sampler(dict(type="concat", model_samplers=[dict(type="anchor", anchors=[_SUB])]))
    with pytest.raises(ValueError, match="fixed teacher"):
        SandwichHook(concat).before_run(runner)


def test_finetune_model_space_with_a_distiller_is_order_independent(tmp_path):
    from gaia_seg_amd.apis.finetune import finetune_model_space
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    cfg = Config(dict(optimizer=dict(type="SGD", lr=0.02, momentum=0.9, weight_decay=1e-4),
                      optimizer_config=dict(), lr_config=dict(policy="poly", power=0.9, min_lr=1e-4,
                                                              by_epoch=False),
                      runner=dict(type="IterBasedRunner", max_iters=2), data=dict(samples_per_gpu=2)))

    def meta(label, arch):
        a = ARCHS[arch]
        return {"name": label, "arch.backbone.stem.width": a["stem"],
                "arch.backbone.body.width": tuple(a["width"]), "arch.backbone.body.depth": tuple(a["depth"])}
    A, B = meta("A", "sub"), meta("B", "min")

    def run(metas):
        model = build_segmentor(distiller_cfg(str(ck), student_os8=True))
        randomize(model, 5)
        rows = finetune_model_space(model.cuda().train(), metas, cfg, _batches((3, 4)), _batches((11, 12)), 2)
        return {r["name"]: r for r in rows}
    ab, ba = run([A, B]), run([B, A])
    assert ab == ba and set(ab) == {"A", "B"}
    assert all(np.isfinite(ab[k]["metric.finetune.mIoU"]) for k in ab)


def test_train_supernet_cli_with_the_distiller_config(tmp_path):
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_segmentor
    cfg_path = os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller.py")
    cfg = Config.fromfile(cfg_path)
    # (a shallow teacher keeps the checkpoint the test writes small; the config's own is the MAX net)
    depth = "model.teacher_segmentor.backbone.body_depth=[2,2,5,2]"
    cfg.merge_from_dict({"model.teacher_segmentor.backbone.body_depth": [2, 2, 5, 2]})
    tcfg = copy.deepcopy(dict(cfg.model["teacher_segmentor"]))
    assert tcfg["backbone"]["body_depth"] == [2, 2, 5, 2]
    tcfg["test_cfg"] = dict(mode="whole")
    teacher = build_segmentor(tcfg)                  # a fresh model's weights
    ck = str(tmp_path / "teacher.pth")
    save_checkpoint(teacher, ck)
    del teacher
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_supernet.py"), cfg_path,
           "--work-dir", str(tmp_path), "--seed", "0", "--no-validate", "--max-iters", "2",
           "--cfg-options", "data.train.size=(64,128)", "log_config.interval=1",
           "checkpoint_config.interval=2", "model.teacher_ckpt=%s" % ck, depth]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stderr + res.stdout
    assert "Iter [2/2]" in out and "finished 2 iterations" in out
    for key in ("distill_loss_seg", "pairwise_loss_seg", "aux.loss_seg", " loss_seg"):
        assert key in out, key
    saved = torch.load(os.path.join(str(tmp_path), "iter_2.pth"), map_location="cpu")
    assert not any(k.startswith("teacher_segmentor") for k in saved["state_dict"])
    plain = build_segmentor(Config.fromfile(os.path.join(ROOT, "configs", "supernet",
                                                         "pspnet_ar50to101v2.py")).model)
    assert list(saved["state_dict"]) == list(plain.state_dict())
