"""DynamicDistiller without a GPU: registry and constructor, the unregistered teacher, the C-ABI rows
of the two new operators, the window draw, and the torch restatement of both losses
(tests/util_distiller.py) against what the reference's own methods produced
(tests/golden/ref_distiller.npz, written by tests/golden/make_ref_distiller_fixtures.py)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import util_distiller as U  # noqa: E402
from util_models import model_cfg, psp_head, tiny_backbone  # noqa: E402


def teacher_cfg(os8=True, num_classes=19):
    """A teacher of other widths (last stage 320 channels) and, by default, another output stride."""
    bk = tiny_backbone(os8=os8)
    bk.update(body_width=[16, 32, 48, 80], stem_width=16)
    head = psp_head(in_channels=320, channels=32)
    head["num_classes"] = num_classes
    return dict(type="DynamicEncoderDecoder", backbone=bk, decode_head=head, train_cfg=dict())


def distiller_cfg(teacher_ckpt, teacher=None, student_os8=False, **kw):
    cfg = model_cfg(psp_head(), aux=True, os8=student_os8)
    cfg.update(type="DynamicDistiller", teacher_segmentor=teacher or teacher_cfg(),
               teacher_ckpt=teacher_ckpt, **kw)
    return cfg


def write_teacher(path, cfg=None, seed=1):
    from util_models import randomize
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    cfg = copy.deepcopy(cfg or teacher_cfg())
    cfg["test_cfg"] = dict(mode="whole")
    t = build_segmentor(cfg)
    randomize(t, seed)
    save_checkpoint(t, str(path))
    return t


@pytest.fixture(scope="module")
def fx():
    return np.load(U.FIXTURE)


def test_registry_and_constructor_validation(tmp_path):
    from gaia_seg_amd.models import SEGMENTORS, build_segmentor
    assert "DynamicDistiller" in SEGMENTORS.module_dict
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    with pytest.raises(AssertionError, match="Teacher ckpt is missed"):
        build_segmentor(distiller_cfg(None))
    with pytest.raises(FileNotFoundError):
        build_segmentor(distiller_cfg(str(tmp_path / "nowhere.pth")))
    with pytest.raises(ValueError, match="classes"):
        build_segmentor(distiller_cfg(str(ck), teacher=teacher_cfg(num_classes=7)))
    # both flags off: no teacher is built and no checkpoint is needed
    m = build_segmentor(distiller_cfg(None, has_distill_loss=False, has_pairwise_loss=False))
    assert m.teacher_segmentor is None
    m = build_segmentor(distiller_cfg(str(ck), distill_loss_temperature=2.5, pairwise_loss_weight=0.5))
    t = m.teacher_segmentor
    assert t is not None and not t.training and not any(p.requires_grad for p in t.parameters())
    assert (m.distill_loss_temperature, m.pairwise_loss_weight) == (2.5, 0.5)
    m.train()
    assert m.training and not t.training and not any(s.training for s in t.modules())


def test_teacher_is_outside_module_registration(tmp_path):
    from gaia_seg_amd.core.checkpoint import load_checkpoint, save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    teacher0 = write_teacher(ck)
    m = build_segmentor(distiller_cfg(str(ck)))
    plain = build_segmentor(model_cfg(psp_head(), aux=True))
    assert list(m.state_dict()) == list(plain.state_dict())
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in plain.named_parameters()]
    t = m.teacher_segmentor
    t_ids = {id(p) for p in t.parameters()} | {id(b) for b in t.buffers()}
    assert t_ids and not t_ids & {id(p) for p in m.parameters()}
    assert not t_ids & {id(b) for b in m.buffers()}
    assert not t_ids & {id(p) for p in m.active_parameters()}
    assert all(mod is not t for mod in m.modules())
    assert not any(k.startswith("teacher_segmentor") for k in m.state_dict())
    # the teacher holds the checkpoint's weights
    for k, v in teacher0.state_dict().items():
        assert torch.equal(t.state_dict()[k], v), k
    # a checkpoint in mmcv's form (teacher keys inside) loads into the distiller and into a plain model
    sd = dict(plain.state_dict())
    sd.update({"teacher_segmentor." + k: v for k, v in teacher0.state_dict().items()})
    path = tmp_path / "mmcv_style.pth"
    torch.save(dict(state_dict=sd, meta={}), str(path))
    load_checkpoint(m, str(path), strict=True)
    load_checkpoint(plain, str(path), strict=True)
    # ... and what this build saves holds the student only
    save_checkpoint(m, str(tmp_path / "student.pth"))
    saved = torch.load(str(tmp_path / "student.pth"), map_location="cpu")["state_dict"]
    assert list(saved) == list(plain.state_dict())


def test_sandwich_with_a_fixed_teacher_is_refused_and_steps_are_never_captured(tmp_path):
    from gaia_seg_amd.core.runner import check_sandwich_model
    from gaia_seg_amd.models import build_segmentor
    m = build_segmentor(distiller_cfg(None, has_distill_loss=False, has_pairwise_loss=False))
    with pytest.raises(ValueError, match="fixed teacher"):
        check_sandwich_model(m)
    check_sandwich_model(build_segmentor(model_cfg(psp_head(), aux=True)))   # (the plain model passes)
    assert m.step_graph_capturable is False


def test_header_and_binding_rows():
    from gaia_seg_amd.hip import lib
    names = {"gs_distill_workspace_bytes", "gs_distill_forward", "gs_distill_backward_workspace_bytes",
             "gs_distill_backward", "gs_pairwise_save_bytes", "gs_pairwise_forward", "gs_pairwise_backward"}
    assert names <= set(lib.PROTOTYPES)
    header = open(os.path.join(lib.REPO_ROOT, "include", "gaiaseg_hip.h")).read()
    assert "#define GS_PAIRWISE_MAX_P %d" % lib.PAIRWISE_MAX_P in header and lib.PAIRWISE_MAX_P >= 128
    assert ctypes.sizeof(lib.DistillDesc) == 8 * 4 + 8 * 8 + 2 * 4
    assert ctypes.sizeof(lib.PairwiseDesc) == 12 * 4 + 8 * 8 + 2 * 4
    assert ctypes.sizeof(lib.KdDesc) == 6 * 4 + 8 * 8 + 4 * 4     # (unchanged)
    L = lib.load()
    d = lib.PairwiseDesc()
    d.N, d.Cs, d.Ct, d.H, d.W, d.Ht, d.Wt, d.T = 1, 8, 8, 300, 4, 300, 4, 1.0
    d.y0, d.y1, d.x0, d.x1 = 0, lib.PAIRWISE_MAX_P, 2, 3
    p = lib.PAIRWISE_MAX_P
    assert L.gs_pairwise_save_bytes(ctypes.byref(d)) == 8 + 4 * (3 * p * p + 5 * p)
    d.y1 = lib.PAIRWISE_MAX_P + 1     # above the cap: refused before any launch (no GPU here)
    assert L.gs_pairwise_save_bytes(ctypes.byref(d)) == 0
    assert L.gs_pairwise_forward(ctypes.byref(d), None, None, 1.0, None, None, 0, None) == -1
    assert L.gs_pairwise_backward(ctypes.byref(d), None, None, 0, 1.0, None, 8, None) == -1
    d.y1, d.x1 = 4, 5                 # the window leaves the map
    assert L.gs_pairwise_forward(ctypes.byref(d), None, None, 1.0, None, None, 0, None) == -1
    q = lib.DistillDesc()
    assert L.gs_distill_workspace_bytes(ctypes.byref(q)) == 0
    assert L.gs_distill_forward(ctypes.byref(q), None, None, None, None, 1.0, None, None, 0, None) == -1
    q.N, q.Cls, q.hs, q.ws, q.ht, q.wt, q.H, q.W, q.T = 2, 19, 5, 7, 9, 13, 33, 49, 1.0
    k = lib.KdDesc()
    k.N, k.Cls, k.h, k.w, k.H, k.W, k.T, k.interpolation = 2, 19, 5, 7, 33, 49, 1.0, 1
    assert L.gs_distill_workspace_bytes(ctypes.byref(q)) == L.gs_kd_workspace_bytes(ctypes.byref(k)) > 0
    assert (L.gs_distill_backward_workspace_bytes(ctypes.byref(q), 20)
            == L.gs_kd_backward_workspace_bytes(ctypes.byref(k), 20) > 0)
    assert L.gs_distill_forward(ctypes.byref(q), None, None, None, None, 1.0, None, None, 0, None) == -4


def test_window_draw_reproduces_the_reference_arithmetic(fx):
    from gaia_seg_amd.apis.train import set_random_seed
    from gaia_seg_amd.models.losses.distill_loss import draw_pairwise_window
    for tag, case in U.PAIRWISE_CASES.items():
        h, w, seed = case[3], case[4], case[7]
        set_random_seed(seed)
        win = draw_pairwise_window(h, w)
        assert win == tuple(int(v) for v in fx["pw_%s_window" % tag]) == U.window_of(h, w, seed)
        y0, y1, x0, x1, sh, sw = win
        assert (sh, sw) == (int(.5 * h), int(.5 * w)) and y1 - y0 == sh and x1 == x0 + 1
        assert 0 <= y0 and y1 <= h and sw <= x0 < w
    # h first, then w: the two draws in order
    np.random.seed(3)
    ch, cw = np.random.uniform(0, .5), np.random.uniform(0, .5)
    np.random.seed(3)
    win = draw_pairwise_window(40, 64)
    assert (win[0], win[2]) == (int(ch * 40), int(cw * 64) + 32)
    assert tuple(int(v) for v in fx["pw_prod_window"]) == U.production_inputs()[2]


@pytest.mark.parametrize("tag", list(U.PAIRWISE_CASES))
def test_pairwise_restatement_equals_the_reference(fx, tag):
    n, cs, ct, h, w, T, wgt, seed, nonc = U.PAIRWISE_CASES[tag]
    win = tuple(int(v) for v in fx["pw_%s_window" % tag])
    y0, y1, x0 = win[:3]
    for dt, suffix, tol in ((torch.float64, "64", 1e-12), (torch.float32, "32", 1e-5)):
        s = U.embed_window(torch.from_numpy(fx["pw_%s_s" % tag]).to(dt), h, w, win, seed + 100, nonc)
        t = U.embed_window(torch.from_numpy(fx["pw_%s_t" % tag]).to(dt), h, w, win, seed + 200)
        assert s.is_contiguous() is False and (s.stride(1) == 1)
        loss, grad = U.loss_and_grad(U.ref_pairwise_loss, s, t, win, T, wgt)
        ref_l, ref_g = float(fx["pw_%s_loss%s" % (tag, suffix)]), torch.from_numpy(fx["pw_%s_grad%s" % (tag, suffix)])
        assert abs(float(loss) - ref_l) <= tol * abs(ref_l)
        gw = grad[:, :, y0:y1, x0]
        assert float((gw.double() - ref_g.double()).abs().max()) <= tol * float(ref_g.abs().max())
        mask = torch.ones(h, w, dtype=torch.bool)
        mask[y0:y1, x0] = False
        assert (grad[:, :, mask] == 0).all() and torch.isfinite(grad).all()
    if tag == "zero":   # the condition this case is there for
        assert (fx["pw_zero_s"][0, :, 1] == 0).all() and (fx["pw_zero_t"][1, :, 2] == 0).all()


@pytest.mark.parametrize("tag", list(U.DISTILL_CASES))
def test_distill_restatement_equals_the_reference(fx, tag):
    n, c, hs, ht, hw, align, T, wgt = U.DISTILL_CASES[tag]
    s64 = torch.from_numpy(fx["kd_%s_s" % tag]).double()
    t64 = torch.from_numpy(fx["kd_%s_t" % tag]).double()
    assert tuple(s64.shape) == (n, c) + hs and tuple(t64.shape) == (n, c) + ht
    loss, grad = U.loss_and_grad(U.ref_distill_loss, s64, t64, hw, T, wgt, align)
    ref_l, ref_g = float(fx["kd_%s_loss64" % tag]), torch.from_numpy(fx["kd_%s_grad64" % tag])
    assert abs(float(loss) - ref_l) <= 1e-12 * abs(ref_l)
    assert float((grad - ref_g).abs().max()) <= 1e-12 * float(ref_g.abs().max())
    loss32, _ = U.loss_and_grad(U.ref_distill_loss, s64.float(), t64.float(), hw, T, wgt, align)
    assert abs(float(loss32) - float(fx["kd_%s_loss32" % tag])) <= 1e-5 * abs(ref_l)


def test_fixture_is_small():
    assert os.path.getsize(U.FIXTURE) < 200 * 1024
