"""Channel-wise distillation on the MI355X: the operator (csrc/cwd.hip gs_cwd_*) against the fp64
restatement of tests/util_cwd.py, its exact-zero and reproducibility contracts, and the DynamicDistiller
/ runner / fast-finetune plumbing around `channel_loss_seg`.

Bounds: the bar of the sibling operators (tests/test_distiller_gpu.py): loss within 1e-5 relative,
gradient within 1e-5 of the largest reference gradient in the max norm, or, where that is larger, 4x
the error of torch's fp32 CPU evaluation of the same formula against fp64 on the same inputs."""
import copy
import ctypes
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import util_cwd as U  # noqa: E402
from test_distiller import distiller_cfg, teacher_cfg, write_teacher  # noqa: E402
from util_models import ARCHS, arch_meta, make_batch, model_cfg, psp_head, randomize  # noqa: E402

PROFILE = os.environ.get("GS_CWD_ERRORS")   # path: one JSON line of observed errors per case
ONLY_CHANNEL = dict(has_distill_loss=False, has_pairwise_loss=False, has_channel_loss=True)


def _note(**rec):
    print("[cwd] " + json.dumps(rec))
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _case(tag):
    return U.CASES.get(tag) or U.ZERO_CASES[tag]


def _run(tag, upstream=1.0):
    from gaia_seg_amd.models.losses.distill_loss import channel_distill_loss
    T, wgt = _case(tag)[5], _case(tag)[6]
    s, t = U.upload(tag)
    s = s.detach().requires_grad_(True)
    loss = channel_distill_loss(s, t, T=T, weight=wgt)
    (loss * upstream).backward()
    assert t.grad is None and not t.requires_grad                # the teacher gets no gradient
    return float(loss), s.grad.detach().clone()


# ---- the operator against fp64 -------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(U.CASES))
def test_op_matches_fp64(tag):
    l64, g64, ref_el, ref_eg = U.reference(tag)
    loss, grad = _run(tag)
    e_l = abs(loss - l64) / abs(l64)
    e_g = float((grad.double().cpu() - g64).abs().max() / g64.abs().max())
    _note(op="cwd", case=tag, loss_relerr=e_l, grad_relerr=e_g, ref32_loss_relerr=ref_el,
          ref32_grad_relerr=ref_eg)
    assert math.isfinite(loss) and torch.isfinite(grad).all()
    assert e_l <= max(1e-5, 4 * ref_el), (loss, l64, e_l, ref_el)
    assert e_g <= max(1e-5, 4 * ref_eg), (e_g, ref_eg)


def test_images_of_a_batch_are_independent():
    """N = 2 with different data per image: each image's gradient is what that image alone gives (at
    twice the weight: the divisor is N * C)."""
    from gaia_seg_amd.models.losses.distill_loss import channel_distill_loss
    tag = "c19_p517"
    T, wgt = _case(tag)[5], _case(tag)[6]
    _, both = _run(tag)
    s, t = U.upload(tag)
    assert not torch.equal(s[0], s[1])
    for i in range(2):
        si = s[i:i + 1].detach().requires_grad_(True)
        channel_distill_loss(si, t[i:i + 1], T=T, weight=wgt / 2).backward()
        assert torch.equal(si.grad[0], both[i])


@pytest.mark.parametrize("tag", list(U.ZERO_CASES))
def test_exact_zeros(tag):
    """A 1 x 1 map, and a teacher that holds the student's values in the student's layout: loss exactly
    0.0 and gradient exactly 0 (both sides run the same arithmetic)."""
    loss, grad = _run(tag)
    _note(op="cwd", case=tag, loss=loss, grad_absmax=float(grad.abs().max()))
    assert loss == 0.0
    assert (grad == 0).all()


def _direct(tag, scale=0.25, ld_extra=0):
    """(loss, lse_s, lse_t, dense gradient incl. pad columns) through the C-ABI."""
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import cwd_desc
    L = lib.load()
    n, c, h, w, _layout, T = _case(tag)[:6]
    s, t = U.upload(tag)
    d = cwd_desc(s, t, T)
    ld = U.round_up(c, 4) + ld_extra
    lse_s = torch.full((n, c), 7.0, device="cuda")
    lse_t = torch.full((n, c), 7.0, device="cuda")
    out = torch.full((1,), 7.0, device="cuda")
    need = L.gs_cwd_workspace_bytes(ctypes.byref(d))
    assert need > 0
    ws = torch.empty(need // 4, device="cuda")
    assert L.gs_cwd_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(),
                            scale, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) == 0
    buf = torch.full((n, h, w, ld), 7.0, device="cuda")
    assert L.gs_cwd_backward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                             lse_t.data_ptr(), scale, buf.data_ptr(), ld, None) == 0
    torch.cuda.synchronize()
    return out.clone(), lse_s, lse_t, buf


@pytest.mark.parametrize("tag", ["c19_p517", "c150", "nchw_c19", "c3"])
def test_launches_are_bitwise_reproducible_and_zero_the_pad(tag):
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import cwd_desc
    c = _case(tag)[1]
    a, b = _direct(tag), _direct(tag)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    out, lse_s, lse_t, buf = a
    assert torch.isfinite(lse_s).all() and torch.isfinite(lse_t).all()
    assert (buf[..., c:] == 0).all() and buf[..., :c].any()
    wide = _direct(tag, ld_extra=4)[3]                           # a wider gradient buffer: same values
    assert torch.equal(wide[..., :c], buf[..., :c]) and (wide[..., c:] == 0).all()
    # the stats are the log-sum-exp of each class map
    s, t = U.upload(tag)
    T = _case(tag)[5]
    want = torch.logsumexp(s.double().flatten(2) / T, dim=2)
    assert float((lse_s.double() - want).abs().max()) <= 1e-5 * float(want.abs().max().clamp(min=1))
    if tag != "c3":   # these cases cross the multi-workgroup combine
        assert lib.load().gs_cwd_debug_partials(ctypes.byref(cwd_desc(s, t, T))) >= 2


def test_split_sizes_on_the_device_tensors():
    """The views the operator tests upload give the split the case table claims."""
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import cwd_desc
    L = lib.load()
    parts = {}
    for tag in ("c19_p63", "c19_p258", "c19_p517"):
        s, t = U.upload(tag)
        assert s.stride(3) == 20 and t.stride(3) == 24 and s.stride(1) == 1
        assert (s[:, :, 0, 0].cpu() != 3.25).all()
        parts[tag] = L.gs_cwd_debug_partials(ctypes.byref(cwd_desc(s, t, 1.0)))
    assert parts["c19_p63"] == 1 and parts["c19_p258"] >= 2 and parts["c19_p517"] >= 3
    n, c, h, w = _case("c19_p517")[:4]
    assert (h * w) % -(-(h * w) // parts["c19_p517"]) != 0


def test_upstream_scalar_scales_the_gradient_exactly():
    _, g1 = _run("c19_p258")
    _, g512 = _run("c19_p258", upstream=512.0)
    assert torch.equal(g512, g1 * 512.0) and g1.abs().max() > 0


def test_validation_on_the_device():
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import channel_distill_loss, cwd_desc
    L = lib.load()
    s = torch.randn(2, 19, 8, 8, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match=r"\(2, 19, 8, 8\).*\(2, 19, 4, 4\)"):
        channel_distill_loss(s, torch.randn(2, 19, 4, 4, device="cuda"))
    with pytest.raises(ValueError, match=r"\(2, 19, 8, 8\).*\(2, 7, 8, 8\)"):
        channel_distill_loss(s, torch.randn(2, 7, 8, 8, device="cuda"))
    with pytest.raises(TypeError):
        channel_distill_loss(s, torch.randn(2, 19, 8, 8, device="cuda").half())
    t = torch.randn(2, 19, 8, 8, device="cuda")
    d = cwd_desc(s, t, 1.0)
    lse = torch.empty(2, 19, device="cuda")
    out = torch.empty(1, device="cuda")
    ws = torch.empty(L.gs_cwd_workspace_bytes(ctypes.byref(d)) // 4, device="cuda")
    args = (s.data_ptr(), t.data_ptr(), lse.data_ptr(), lse.data_ptr(), 1.0, out.data_ptr())
    assert L.gs_cwd_forward(ctypes.byref(d), *args, ws.data_ptr(), 16, None) == -3
    assert L.gs_cwd_forward(ctypes.byref(d), *args, None, ws.numel() * 4, None) == -4
    d.T = 0.0
    assert L.gs_cwd_forward(ctypes.byref(d), *args, ws.data_ptr(), ws.numel() * 4, None) == -1
    with pytest.raises(lib.HipLibraryError):
        channel_distill_loss(s, t, T=0.0)


# ---- the segmentor -------------------------------------------------------------------------------
def test_channel_loss_train_step_against_the_oracle(tmp_path):
    """One train step with the channel loss alone against oracle student + oracle teacher + the fp64
    restatement, under the criteria of tests/parity.py."""
    import parity
    from oracle.model import OEncoderDecoder
    from test_distiller_gpu import ODistiller
    from gaia_seg_amd.models import build_segmentor

    class OChannel(ODistiller):
        def forward_train(self, img, gt):
            from oracle import ops as O
            ctx, O._RELU_CTX = O._RELU_CTX, None
            try:
                with torch.no_grad():
                    t = self.teacher.decode_head(self.teacher.backbone(img))
            finally:
                O._RELU_CTX = ctx
            x = self.backbone(img)
            s = self.decode_head(x)
            losses = dict(self.decode_head.losses(s, gt))
            losses["channel_loss_seg"] = U.ref_channel_loss(s, t.to(s.dtype), 2.0, 5.0)
            losses.update({"aux." + k: v for k, v in self.auxiliary_head.forward_train(x, gt).items()})
            return losses

    ck = tmp_path / "teacher.pth"
    tcfg = teacher_cfg(os8=True)
    t_prod = write_teacher(ck, tcfg)
    prod = build_segmentor(distiller_cfg(str(ck), teacher=tcfg, student_os8=True, channel_loss_temperature=2,
                                         channel_loss_weight=5, **ONLY_CHANNEL))
    randomize(prod, 0)
    scfg = model_cfg(psp_head(), aux=True, os8=True)
    o_student = OEncoderDecoder(**{k: v for k, v in copy.deepcopy(scfg).items() if k != "type"})
    o_student.load_state_dict({k: v.detach().clone().contiguous() for k, v in prod.state_dict().items()})
    o_teacher = OEncoderDecoder(**{k: v for k, v in copy.deepcopy(tcfg).items() if k != "type"})
    o_teacher.load_state_dict({k: v.detach().clone().contiguous() for k, v in t_prod.state_dict().items()})
    prod = prod.cuda().train()
    prod.manipulate_arch(arch_meta("sub"))
    o_student.manipulate_arch(arch_meta("sub"))
    img, gt = make_batch(2, 64, 64, seed=2)
    orc = OChannel(o_student, o_teacher, None).train()
    errs = parity.train_step_parity(prod, orc, img, gt)
    assert errs["loss"] < parity.TOL


def test_loss_keys_with_the_flag_on_and_off(tmp_path):
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    img, gt = make_batch(2, 64, 64, seed=2)
    batch = dict(img=img.cuda(), img_metas=[{}] * 2, gt_semantic_seg=gt.cuda())
    off = build_segmentor(distiller_cfg(str(ck), student_os8=True))
    randomize(off, 0)
    np.random.seed(3)
    out = off.cuda().train().train_step(batch, None)
    assert "channel_loss_seg" not in out["log_vars"]
    on = build_segmentor(distiller_cfg(str(ck), student_os8=True, **ONLY_CHANNEL))
    randomize(on, 0)
    on = on.cuda().train()
    out = on.train_step(batch, None)
    assert list(out["log_vars"]) == ["loss_seg", "acc_seg", "channel_loss_seg", "aux.loss_seg",
                                     "aux.acc_seg", "loss"]
    lv = out["log_vars"]
    assert torch.equal(out["loss"].detach(), (lv["loss_seg"] + lv["channel_loss_seg"]) + lv["aux.loss_seg"])
    assert float(lv["channel_loss_seg"]) > 0
    out["loss"].backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in on.teacher_segmentor.parameters())
    # a teacher at another output stride: refused at the first step, with both shapes
    mixed = build_segmentor(distiller_cfg(str(ck), student_os8=False, **ONLY_CHANNEL))
    randomize(mixed, 0)
    with pytest.raises(ValueError, match=r"\(2, 19, 2, 2\).*\(2, 19, 8, 8\)"):
        mixed.cuda().train().train_step(batch, None)


_SUB = {"name": "SUB", "arch.backbone.stem.width": ARCHS["sub"]["stem"],
        "arch.backbone.body.width": list(ARCHS["sub"]["width"]),
        "arch.backbone.body.depth": list(ARCHS["sub"]["depth"])}
# the keys configs/supernet/pspnet_ar50to101v2_distiller_cwd.py sets
CWD_KEYS = dict(has_pairwise_loss=False, has_channel_loss=True, channel_loss_temperature=1,
                channel_loss_weight=5)


def _runner(model, optimizer_config):
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core import dist as gdist
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, IterBasedRunner, ManipulateArchHook
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments, bucket_bytes=1 << 20),
                             base_lr=0.05, momentum=0.9, weight_decay=5e-4, max_iters=100)
    runner.register_hook(ManipulateArchHook(build_model_sampler(dict(type="anchor", anchors=[_SUB]))))
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(optimizer_hook(optimizer_config))
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


@pytest.mark.parametrize("optimizer_config", [dict(), dict(type="Fp16OptimizerHook", loss_scale=512.)],
                         ids=["fp32", "fp16_scale512"])
def test_three_runner_iterations_with_the_config_keys(tmp_path, optimizer_config):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller_cwd.py"))
    assert {k: cfg.model[k] for k in CWD_KEYS} == CWD_KEYS
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    model = build_segmentor(distiller_cfg(str(ck), student_os8=True, **CWD_KEYS))
    randomize(model, 3)
    runner, arena = _runner(model.cuda().train(), optimizer_config)
    p0 = arena.flat_param.clone()
    for batch in _batches((1, 2, 3)):
        out = runner.train_iter(batch)
        assert "channel_loss_seg" in out["log_vars"] and "pairwise_loss_seg" not in out["log_vars"]
        assert math.isfinite(float(out["log_vars"]["channel_loss_seg"]))
        assert torch.isfinite(out["loss"]).item()
    torch.cuda.synchronize()
    assert torch.isfinite(arena.flat_param).all() and not torch.equal(p0, arena.flat_param)


def test_finetune_supernet_tool_with_the_channel_loss(tmp_path):
    """One tools/finetune_supernet.py turn whose `model` carries the config's keys."""
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    tck = tmp_path / "teacher.pth"
    write_teacher(tck)
    mcfg = distiller_cfg(str(tck), student_os8=True, **CWD_KEYS)
    src = build_segmentor(copy.deepcopy(model_cfg(psp_head(), aux=True, os8=True)))
    randomize(src, 5)
    ck = str(tmp_path / "supernet.pth")
    save_checkpoint(src, ck, meta=dict(iter=7))
    cfg_path = tmp_path / "tiny_finetune.py"
    cfg_path.write_text(
        "model = %r\n"
        "data = dict(samples_per_gpu=2, workers_per_gpu=2,\n"
        "            train=dict(type='SyntheticSegDataset', size=(64, 64), num_classes=19))\n"
        "optimizer = dict(type='SGD', lr=0.02, momentum=0.9, weight_decay=1e-4)\n"
        "optimizer_config = dict()\n"
        "lr_config = dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False)\n"
        "runner = dict(type='IterBasedRunner', max_iters=2)\n"
        "evaluation = dict(interval=100, metric='mIoU', num_batches=2)\n"
        "log_config = dict(interval=1)\n" % (mcfg,))
    space = tmp_path / "space.json"
    space.write_text(json.dumps([dict(_SUB, **{"metric.direct.mIoU": 0.2})]))
    spec = importlib.util.spec_from_file_location("finetune_supernet_tool",
                                                  os.path.join(ROOT, "tools", "finetune_supernet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main([str(cfg_path), "--load-from", ck, "--model-space-path", str(space),
               "--work-dir", str(tmp_path / "w"), "--seed", "0", "--no-validate"])
    rows = json.load(open(tmp_path / "w" / "finetune_supernet" / "metrics.json"))
    assert [r["name"] for r in rows] == ["SUB"]
    assert math.isfinite(rows[0]["metric.finetune.mIoU"]) and 0.0 <= rows[0]["metric.finetune.mIoU"] <= 1.0
