"""The BEiT backbone on the GPU against the float64 restatement of tests/util_beit.py carrying the same
weights: a tiny model (embed 128, 2 heads, depth 4, out_indices [0, 1, 2, 3], init_values 0.1, qkv_bias)
whose tables, gamma_*, q_bias / v_bias and fpn1 BatchNorm statistics are randomised (the constructor leaves
the tables at zero, which would hide the bias).  Feature maps at the feature bound of
tests/test_elastic_vit_gpu.py (1e-3 in conftest.rel_err).

The patch-8 variant runs at 32 x 48 (window 4 x 6), not at 16 x 24: a 2 x 3 map has no 4 / 4 max-pool
output, so no stride-32 map exists at that size (util_beit.VARIANTS).

Then the module as what it is for: the frozen teacher of a DynamicDistiller over the tiny ViT student of
tests/util_vit.py (one runner step), and a BEiT segmentor evaluated with a sliding window of img_size."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_beit as B
import util_vit as U
from util_models import make_batch, uper_head

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
H, W = 64, 96      # the distiller / evaluation image: a 4 x 6 window, so that the stride-32 maps are 2 x 3


def make_backbone(variant, seed=0, **kw):
    from gaia_seg_amd.models import build_backbone
    m = build_backbone(dict(B.tiny_cfg(variant), **kw))
    B.randomize_beit(m, seed)
    return m.eval()


@pytest.mark.parametrize("variant", list(B.VARIANTS))
def test_feature_maps_against_float64(hip_lib, variant):
    cfg = B.tiny_cfg(variant)
    h, w = cfg["img_size"]
    m = make_backbone(variant)
    assert bool(m.blocks[0].attn.relative_position_bias_table.any()) if cfg.get("use_rel_pos_bias") else \
        bool(m.rel_pos_bias.relative_position_bias_table.any())
    img = make_batch(2, h, w, seed=1)[0]
    want = B.beit_ref(B.double_sd(m), img.double(), cfg)
    m = m.to(DEV)
    with torch.no_grad():
        outs = m(img.to(DEV))
        again = m(img.to(DEV))
    assert [tuple(o.shape) for o in outs] == [(2, 128, max(h // s, 1), max(w // s, 1)) for s in (4, 8, 16, 32)]
    assert [tuple(o.shape) for o in outs] == [tuple(r.shape) for r in want]
    for i, (o, a, r) in enumerate(zip(outs, again, want)):
        err = rel_err(o, r)
        print("%s: map %d (stride %d) rel_err %.3g" % (variant, i, 4 << i, err))
        assert torch.equal(o, a), "map %d differs between two runs" % i
        assert err <= TOL, i


def test_an_input_of_another_size_is_refused(hip_lib):
    m = make_backbone("p16-block-tables").to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="img_size"):
        m(torch.zeros(1, 3, 32, 32, device=DEV))


def test_forward_under_a_recording_tape_with_a_trainable_parameter_raises(hip_lib):
    from gaia_seg_amd.hip.runtime import Act, Tape
    m = make_backbone("p16-block-tables").to(DEV)
    img = torch.zeros(1, 3, 32, 48, device=DEV)
    assert any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match="BEiT: forward only \\(frozen teacher\\)"):
        m(img)                                            # grad mode on, trainable parameters
    with pytest.raises(NotImplementedError, match="BEiT: forward only \\(frozen teacher\\)"):
        m.forward_act(Tape(), Act.from_nchw(img))         # a recording tape
    for p in m.parameters():
        p.requires_grad_(False)
    assert len(m(img)) == 4                               # frozen: nothing is recorded
    with pytest.raises(NotImplementedError, match="forward only"):
        m(img.clone().requires_grad_(True))


# ---- the teacher of a distiller --------------------------------------------------------------------------
def teacher_cfg():
    head = uper_head(in_channels=[128] * 4, channels=16)
    return dict(type="EncoderDecoder", backbone=dict(B.tiny_cfg("p16-block-tables"), img_size=(H, W)),
                decode_head=head, train_cfg=dict())


def write_teacher(path, seed=1):
    """a randomised BEiT + UPerHead teacher saved as a checkpoint (relative_position_index keys included)"""
    from util_models import randomize
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.models import build_segmentor
    t = build_segmentor(dict(copy.deepcopy(teacher_cfg()), test_cfg=dict(mode="whole")))
    randomize(t.decode_head, seed)
    B.randomize_beit(t.backbone, seed)
    save_checkpoint(t, str(path))
    saved = torch.load(str(path), map_location="cpu")["state_dict"]
    assert "backbone.blocks.0.attn.relative_position_index" in saved
    return t


def teacher_logits_ref(teacher, img):
    """the teacher's low-resolution logits in float64: tests/util_beit.py's backbone under the CPU oracle's
    UPerHead (oracle/model.py) with the teacher's weights"""
    from oracle.model import _build_head
    head = _build_head(copy.deepcopy(teacher_cfg()["decode_head"])).double().eval()
    head.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu()
                          for k, v in teacher.decode_head.state_dict().items()})
    cfg = teacher_cfg()["backbone"]
    sd = {k: v.cpu() for k, v in B.double_sd(teacher.backbone).items()}
    with torch.no_grad():
        return head(B.beit_ref(sd, img.double().cpu(), cfg))


def student_cfg(ckpt):
    cfg = copy.deepcopy(U.tiny_model_cfg())
    cfg["backbone"]["img_size"] = (H, W)
    cfg["neck"]["scales"] = [4, 2, 1, 0.5]      # the student's last map at the teacher's stride 32
    cfg.update(type="DynamicDistiller", teacher_segmentor=teacher_cfg(), teacher_ckpt=ckpt)
    return cfg


def _batch(seed, h=H, w=W):
    img, gt = make_batch(2, h, w, seed=seed)
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False) for _ in range(2)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def test_distiller_with_a_beit_teacher_end_to_end(hip_lib, tmp_path):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    from gaia_seg_amd.models import build_segmentor
    ck = tmp_path / "beit_teacher.pth"
    written = write_teacher(ck)
    torch.manual_seed(0)
    model = build_segmentor(student_cfg(str(ck)))
    U.randomize_vit(model.backbone, 0)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    model = model.to(DEV).train()
    t = model.teacher_segmentor
    assert type(t.backbone).__name__ == "BEiT" and not t.training and not t.backbone.training
    assert next(t.parameters()).is_cuda and not any(p.requires_grad for p in t.parameters())
    for (k, a), (_, b) in zip(written.state_dict().items(), t.state_dict().items()):
        assert torch.equal(a, b.cpu()), "%s was not loaded from the checkpoint" % k
    before = {k: v.detach().clone() for k, v in t.state_dict().items()}
    # the teacher's logits against the restatement
    batch = _batch(0)
    feats, logits = model.prepare_distill_feature(batch["img"], batch["img_metas"])
    want = teacher_logits_ref(t, batch["img"])
    assert tuple(logits.shape) == tuple(want.shape) == (2, 19, H // 4, W // 4)
    err = rel_err(logits, want)
    print("teacher logits rel_err %.3g" % err)
    assert err <= TOL
    assert [tuple(f.shape[2:]) for f in feats] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    # one runner step
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.05,
                             momentum=0.9, weight_decay=1e-4, max_iters=100)
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    student_before = {k: v.detach().clone() for k, v in model.named_parameters()}
    runner.set_arch(U.arch_meta("sub"))
    np.random.seed(0)
    out = runner.train_iter(batch)
    torch.cuda.synchronize()
    logs = {k: float(v) for k, v in out["log_vars"].items()}
    print(logs)
    for key in ("distill_loss_seg", "pairwise_loss_seg"):
        assert key in logs and np.isfinite(logs[key]), logs
    # (the pairwise window of a 2 x 3 map is a single pixel, whose affinity with itself is 1 in both models)
    assert logs["distill_loss_seg"] > 0 and logs["pairwise_loss_seg"] >= 0, logs
    # the teacher: absent from the arena, unchanged bit for bit
    lo = arena.flat_param.data_ptr()
    hi = lo + arena.flat_param.numel() * 4
    assert all(not (lo <= p.data_ptr() < hi) for p in t.parameters())
    assert not set(arena.segments) & {id(p) for p in t.parameters()}
    assert set(arena.segments) == {id(p) for p in model.parameters()}
    after = t.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert all(p.grad is None for p in t.parameters())
    # the student's active parameters move
    active = {id(p) for p in model.active_parameters()}
    moved = [k for k, p in model.named_parameters() if id(p) in active and not torch.equal(p, student_before[k])]
    still = [k for k, p in model.named_parameters() if id(p) in active and torch.equal(p, student_before[k])]
    assert not still and len(moved) > 60, still


def test_slide_evaluation_of_a_beit_segmentor(hip_lib):
    """evaluate_model in test_cfg.mode='slide' with crop = stride = img_size on an image of 2 x 2 windows.
    Every window is the model on its own, so the labels are the argmax of the restatement's logits resized
    to the window.  Tie pixels are left out: fp32 logits are within TOL of their largest element (the bound
    asserted above), so a pixel whose two largest float64 logits are closer than twice that may legitimately
    go either way."""
    from util_models import randomize
    from gaia_seg_amd.core.config import ConfigDict
    from gaia_seg_amd.core.evaluation import evaluate_model
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(dict(copy.deepcopy(teacher_cfg()), test_cfg=dict(mode="whole")))
    randomize(model.decode_head, 1)
    B.randomize_beit(model.backbone, 1)
    model.decode_head.dropout = None
    model = model.to(DEV).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    model.test_cfg = ConfigDict(mode="slide", crop_size=(H, W), stride=(H, W))
    batch = _batch(5, 2 * H, 2 * W)
    res = evaluate_model(model, [batch], 1, 19)
    assert all(np.isfinite(v) for v in (res["mIoU"], res["aAcc"])), res
    with torch.no_grad():
        labels = model.simple_test_device(batch["img"], batch["img_metas"], rescale=True).cpu()
    assert tuple(labels.shape) == (2, 2 * H, 2 * W) and labels.dtype == torch.int64
    compared = total = 0
    for y0 in (0, H):
        for x0 in (0, W):
            low = teacher_logits_ref(model, batch["img"][:, :, y0:y0 + H, x0:x0 + W])
            full = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
            top2 = full.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 2 * TOL * float(full.abs().max())
            got = labels[:, y0:y0 + H, x0:x0 + W]
            assert torch.equal(got[clear], full.argmax(dim=1)[clear]), (y0, x0)
            compared += int(clear.sum())
            total += clear.numel()
    print("slide: %d of %d pixels compared" % (compared, total))
    assert compared > 0.9 * total
    # the confusion matrix evaluate_model accumulated is that of these labels
    gt = batch["gt_semantic_seg"].cpu()[:, 0]
    valid = gt != 255
    assert abs(res["aAcc"] - float((labels[valid] == gt[valid]).double().mean())) < 1e-6
