"""In-place distillation (sandwich rule) on the MI355X: the fused KD loss kernels against an fp64 CPU
restatement of the reference's formula, the gradient-accumulation kernel, the heads' distillation
branch, one runner sandwich iteration against the members' individual steps, two ranks in lockstep,
and the training CLI with the new config."""
import copy
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_inplace_distill import kd_restated  # noqa: E402


def _padded_logits(n, c, h, w, ld, seed, scale=3.0):
    """[n, c, h, w] view of a padded NHWC buffer (the heads' layout); pad columns hold garbage."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, h, w, ld, generator=g) * scale
    return buf.cuda().permute(0, 3, 1, 2)[:, :c]


def _axis_weights(n_in, n_out, align):
    """[n_out, n_in] bilinear weights of one axis with ATen's fp32 source-coordinate arithmetic (the
    kernels', csrc/resize.h): interpolating an identity in fp32 yields exactly those weights."""
    eye = torch.eye(n_in, dtype=torch.float32).reshape(1, n_in, n_in, 1)
    w = torch.nn.functional.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=align)
    return w[0, :, :, 0].t().double()


def resize64(x, size, align):
    """fp64 bilinear resize whose weights are the fp32 ones (only the logit arithmetic is exact)."""
    ry = _axis_weights(x.shape[2], size[0], align)
    rx = _axis_weights(x.shape[3], size[1], align)
    return torch.einsum("Yy,ncyx,Xx->ncYX", ry, x, rx)


def kd64(s, t, T, weight, divisor, interpolation, size, align):
    if interpolation:
        s, t = resize64(s, size, align), resize64(t, size, align)
    return kd_restated(s, t, T=T, weight=weight, divisor=divisor)


def _ref_grad(s, t, T, weight, divisor, interpolation, size, align):
    s64 = s.detach().double().cpu().requires_grad_(True)
    loss = kd64(s64, t.double().cpu(), T, weight, divisor, interpolation, size, align)
    loss.backward()
    return loss.detach(), s64.grad


# (N, Cls, h, w, H, W, align_corners, T, interpolation, ld_s, ld_t)
KD_CASES = [
    (2, 19, 6, 8, 48, 64, 0, 2.0, True, 20, 20),        # x8 (PSP head at OS8)
    (1, 19, 4, 5, 64, 80, 0, 1.0, True, 20, 24),        # x16 (FCN aux head)
    (2, 7, 3, 4, 96, 128, 0, 4.0, True, 8, 12),         # x32
    (1, 19, 193, 5, 769, 17, 0, 2.0, True, 20, 20),     # config 4: 193 -> 769 (row tiles)
    (2, 19, 7, 9, 56, 72, 1, 2.0, True, 20, 20),        # align_corners = 1
    (1, 7, 13, 11, 49, 43, 1, 4.0, True, 8, 8),         # non-integer ratio, align_corners = 1
    (2, 19, 6, 8, 6, 8, 0, 2.0, False, 20, 20),         # at logit resolution
    (1, 7, 9, 5, 9, 5, 1, 1.0, False, 12, 8),           # ... padded strides differ
]


@pytest.mark.parametrize("case", KD_CASES, ids=lambda c: "N%d_C%d_%dx%d-%dx%d_ac%d_T%g_%s" % (
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], "interp" if c[8] else "lowres"))
def test_kd_op_matches_fp64_restatement(case):
    from gaia_seg_amd.models.losses.distill_loss import kd_loss
    n, c, h, w, H, W, ac, T, interp, lds, ldt = case
    s = _padded_logits(n, c, h, w, lds, 1).requires_grad_(False)
    t = _padded_logits(n, c, h, w, ldt, 2)
    s_leaf = s.detach().clone().requires_grad_(True)  # contiguous NCHW copy
    for student in (s, s_leaf):
        st = student if student is s_leaf else student.detach().requires_grad_(True)
        loss = kd_loss(st, t, (H, W), T=T, distillation_weight=0.5, divisor=1000.0,
                       interpolation=interp, align_corners=bool(ac))
        loss.backward()
        ref_loss, ref_grad = _ref_grad(s, t, T, 0.5, 1000.0, interp, (H, W), bool(ac))
        assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)), (float(loss), float(ref_loss))
        g = st.grad.double().cpu()
        err = (g - ref_grad).abs().max() / ref_grad.abs().max()
        assert err <= 1e-5, float(err)
        assert t.grad is None


def _direct(case, workspace=True):
    """(loss, dense gradient buffer incl. pad columns) through the C-ABI; workspace=False forces the
    gather form of the interpolated backward."""
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import kd_desc
    L = lib.load()
    n, c, h, w, H, W, ac, T, interp, lds, ldt = case
    s = _padded_logits(n, c, h, w, lds, 1)
    t = _padded_logits(n, c, h, w, ldt, 2)
    d = kd_desc(s, t, (H, W), T, ac, interp)
    lse_s = torch.empty(n, d.H, d.W, device="cuda")
    lse_t = torch.empty_like(lse_s)
    out = torch.empty(1, device="cuda")
    ws = torch.empty(max(L.gs_kd_workspace_bytes(ctypes.byref(d)),
                         L.gs_kd_backward_workspace_bytes(ctypes.byref(d), 20)) // 4 + 4, device="cuda")
    assert L.gs_kd_forward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(),
                           0.25, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) == 0
    ld = 20
    buf = torch.full((n, h, w, ld), 7.0, device="cuda")
    assert L.gs_kd_backward(ctypes.byref(d), s.data_ptr(), t.data_ptr(), lse_s.data_ptr(),
                            lse_t.data_ptr(), 0.25, buf.data_ptr(), ld,
                            ws.data_ptr() if workspace else None, ws.numel() * 4 if workspace else 0,
                            None) == 0
    torch.cuda.synchronize()
    return out.clone(), buf


@pytest.mark.parametrize("case", [KD_CASES[0], KD_CASES[3], KD_CASES[5], KD_CASES[6]])
def test_kd_launches_are_bitwise_reproducible_and_zero_the_pad(case):
    l1, g1 = _direct(case)
    l2, g2 = _direct(case)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    c = case[1]
    assert (g1[..., c:] == 0).all()


@pytest.mark.parametrize("case", [KD_CASES[0], KD_CASES[1], KD_CASES[3], KD_CASES[4]])
def test_kd_gather_form_agrees_with_tile_form(case):
    _, gt = _direct(case, workspace=True)
    _, gg = _direct(case, workspace=False)
    c = case[1]
    err = (gt[..., :c] - gg[..., :c]).abs().max() / gt[..., :c].abs().max()
    assert err <= 1e-5, float(err)
    assert (gg[..., c:] == 0).all()


def test_accumulate_kernel_is_the_torch_add_and_clears_the_source():
    from gaia_seg_amd.hip import lib
    L = lib.load()
    g = torch.Generator().manual_seed(5)
    n = 1 << 16
    dst = (torch.randn(n, generator=g)).cuda()
    src = (torch.randn(n, generator=g)).cuda()
    want = dst.clone()
    srcc = src.clone()
    # aligned ranges (float4 path), odd starts / lengths (scalar path), a one-element range
    ranges = [(0, 4096), (4096 + 64, 9000), (10001, 10002), (12345, 20000), (32768, n)]
    for a, b in ranges:
        want[a:b] = want[a:b] + srcc[a:b]
        assert L.gs_grad_accumulate(dst.data_ptr() + 4 * a, src.data_ptr() + 4 * a, b - a, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, want)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    for a, b in ranges:
        mask[a:b] = True
    assert (src[mask] == 0).all() and torch.equal(src[~mask], srcc[~mask])


def test_param_arena_accumulate_round_trip():
    from util_models import model_cfg, psp_head
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(model_cfg(psp_head(), aux=True)).cuda()
    arena = ParamArena(model)
    g = torch.randn(arena.numel, generator=torch.Generator().manual_seed(0)).cuda()
    arena.flat_grad.copy_(g)
    rng = arena.ranges_for(list(model.parameters()))
    arena.accumulate(rng, into="buffer")
    arena.flat_grad.copy_(g)
    arena.accumulate(rng, into="buffer")
    arena.accumulate(rng, into="grad")
    torch.cuda.synchronize()
    assert torch.equal(arena.flat_grad, g + g) and not arena.flat_acc.any()
    with pytest.raises(ValueError):
        arena.accumulate(rng, into="momentum")


# ---- heads ----
def _tiny(head, seed=0):
    from util_models import model_cfg, randomize
    from gaia_seg_amd.models import build_segmentor
    m = build_segmentor(model_cfg(head, aux=True))
    randomize(m, seed)
    return m.cuda().train()


@pytest.mark.parametrize("which,interp", [("decode", False), ("decode", True), ("aux", False), ("aux", True)])
def test_head_distillation_branch_against_restatement(which, interp):
    import torch.nn.functional as F
    from util_models import make_batch, psp_head
    model = _tiny(psp_head())
    img, gt = make_batch(2, 64, 96)
    img, gt = img.cuda(), gt.cuda()
    head = model.decode_head if which == "decode" else model.auxiliary_head
    key, D = head.kd_teacher_key, head.kd_divisor
    assert (key, D) == (("teacher_logits", 1000.0) if which == "decode" else ("aux_teacher_logits", 2000.0))
    with torch.no_grad():
        x = model.extract_feat(img)
    x = [a.detach() for a in x]
    teacher = head.forward(x).detach() * 1.5 + 0.3       # some other logits at the head's resolution
    t_before = teacher.clone()
    kw = {key: teacher, "T": 2.0, "distillation_weight": 0.5, "interpolation": interp,
          "return_logits": True}
    losses = head.forward_train(x, None, gt, None, **kw)
    s = losses["logits"]
    ref = kd64(s.double().cpu(), teacher.double().cpu(), 2.0, 0.5, D, interp, gt.shape[2:], False)
    assert abs(float(losses["loss_seg"]) - float(ref)) <= 1e-5 * abs(float(ref))
    # the TEACHER's accuracy at the label size (mmseg accuracy: % of all label pixels)
    up = F.interpolate(teacher.double().cpu(), size=gt.shape[2:], mode="bilinear", align_corners=False)
    acc = 100.0 * (up.argmax(1) == gt.cpu().squeeze(1)).sum().item() / gt.numel()
    assert abs(float(losses["acc_seg"]) - acc) <= 100.0 / gt.numel() + 1e-4
    # student gradient: conv_seg's bias gradient is the per-class sum of d loss / d logits
    s64 = s.double().cpu().requires_grad_(True)
    kd64(s64, teacher.double().cpu(), 2.0, 0.5, D, interp, gt.shape[2:], False).backward()
    want = s64.grad.sum(dim=(0, 2, 3))
    head.conv_seg.bias.grad = None
    losses["loss_seg"].backward()
    torch.cuda.synchronize()
    got = head.conv_seg.bias.grad[:want.numel()].double().cpu()
    assert ((got - want).abs().max() / want.abs().max()) <= 1e-4
    assert torch.equal(teacher, t_before)


def test_without_kwargs_the_heads_train_on_labels():
    from util_models import make_batch, psp_head
    model = _tiny(psp_head())
    img, gt = make_batch(2, 64, 96)
    out1 = model.train_step(dict(img=img.cuda(), img_metas=[{}] * 2, gt_semantic_seg=gt.cuda()), None)
    assert set(out1) == {"loss", "log_vars", "num_samples"}
    out2 = model.train_step(dict(img=img.cuda(), img_metas=[{}] * 2, gt_semantic_seg=gt.cuda()), None,
                            return_logits=True)
    lg, ag = out2["logits"], out2["aux_logits"]
    assert lg.shape[:2] == (2, 19) and ag.shape == (2, 19, 2 * lg.shape[2], 2 * lg.shape[3])
    assert set(out2["log_vars"]) == set(out1["log_vars"])


# ---- runner ----
_MAXM = {"name": "MAX", "arch.backbone.stem.width": 32, "arch.backbone.body.width": [32, 64, 96, 128],
         "arch.backbone.body.depth": [2, 2, 3, 2]}
_MINM = {"name": "MIN", "arch.backbone.stem.width": 16, "arch.backbone.body.width": [16, 32, 48, 64],
         "arch.backbone.body.depth": [1, 1, 1, 1]}
_SUBM = {"arch.backbone.stem.width": 16, "arch.backbone.body.width": [16, 48, 64, 96],
         "arch.backbone.body.depth": [1, 2, 2, 1]}
_KD = dict(T=2.0, distillation_weight=0.5, interpolation=False)


def _sandwich_runner(model, lr=0.05, kd=_KD, random_member=True):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, IterBasedRunner, SandwichHook
    from gaia_seg_amd.core import dist as gdist
    arena = ParamArena(model)
    gdist.sync_module_states(model, arena)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments, bucket_bytes=1 << 20),
                             base_lr=lr, momentum=0.9, weight_decay=5e-4, max_iters=100)
    rand = (dict(type="anchor", anchors=[_SUBM]) if random_member else dict(type="composite", model_samplers=[
        dict(type="range", key="arch.backbone.stem.width", start=16, end=32, step=16),
        dict(type="candidate", key="arch.backbone.body.width", candidates=[[16, 48, 64, 96], [32, 64, 96, 128]]),
        dict(type="candidate", key="arch.backbone.body.depth", candidates=[[1, 2, 2, 1], [2, 1, 3, 2]])]))
    sampler = build_model_sampler(dict(type="concat", model_samplers=[
        dict(type="anchor", anchors=[_MAXM]), dict(type="anchor", anchors=[_MINM]), rand]))
    sampler.seed(11)
    runner.register_hook(FixedLrUpdaterHook())
    runner.register_hook(SandwichHook(sampler, kd))
    runner.call_hook("before_run")
    return runner, arena


def test_sandwich_iteration_equals_the_sum_of_member_steps():
    from util_models import psp_head
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.synthetic import make_batch
    batch = make_batch(2, 64, 96, seed=3, device="cuda", border=2)
    model_a = _tiny(psp_head(), seed=4)
    model_b = copy.deepcopy(model_a)
    runner, arena = _sandwich_runner(model_a)
    # record what the iteration's one SGD step is given, and clones of the teacher logits
    seen, teacher_clone = {}, {}
    orig_step, orig_train_step = arena.sgd_step, model_a.train_step

    def rec_step(ranges, *a, **k):
        seen["grad"], seen["ranges"], seen["args"] = arena.flat_grad.clone(), list(ranges), (a, k)
        return orig_step(ranges, *a, **k)

    def rec_train_step(data, opt=None, **kw):
        out = orig_train_step(data, opt, **kw)
        if kw.get("return_logits"):
            teacher_clone["t"] = (out["logits"].clone(), out["aux_logits"].clone())
        return out
    arena.sgd_step = rec_step
    model_a.train_step = rec_train_step
    out = runner.train_iter(batch)
    torch.cuda.synchronize()
    assert out["members"] == ["MAX", "MIN", "random0"]
    assert {k.split(".")[0] for k in out["log_vars"] if k != "loss"} == {"MAX", "MIN", "random0"}
    assert "MIN.decode.loss_seg" in out["log_vars"] and "random0.aux.acc_seg" in out["log_vars"]
    parts = [out["log_vars"]["%s.loss" % m] for m in out["members"]]
    assert torch.equal(out["loss"], (parts[0] + parts[1]) + parts[2])
    # the teacher logits were not overwritten by the later members
    t_end = out["teacher_logits"]
    assert torch.equal(t_end[0], teacher_clone["t"][0]) and torch.equal(t_end[1], teacher_clone["t"][1])
    # invariants after the iteration
    assert arena.grads_clean and not arena.flat_grad.any() and not arena.flat_acc.any()

    # the same members, one by one, on a twin model: gradients summed in member order
    arena_b = ParamArena(model_b)
    g_sum, teacher = None, None
    for i, meta in enumerate([_MAXM, _MINM, _SUBM]):
        model_b.manipulate_arch(fold_dict(meta)["arch"])
        arena_b.flat_grad.zero_()
        if i == 0:
            o = model_b.train_step(batch, None, return_logits=True)
            teacher = (o["logits"], o["aux_logits"])
        else:
            o = model_b.train_step(batch, None, teacher_logits=teacher[0], aux_teacher_logits=teacher[1], **_KD)
        o["loss"].backward()
        torch.cuda.synchronize()
        g = arena_b.flat_grad.clone()
        g_sum = g if g_sum is None else g_sum + g
        assert torch.equal(o["loss"].detach(), out["log_vars"]["%s.loss" % ["MAX", "MIN", "random0"][i]])
    assert torch.equal(seen["grad"], g_sum)
    model_b.manipulate_arch(fold_dict(_MAXM)["arch"])
    max_ranges = arena_b.ranges_for([p for p in model_b.active_parameters() if p.requires_grad])
    assert seen["ranges"] == max_ranges
    arena_b.flat_grad.copy_(g_sum)
    arena_b.sgd_step(max_ranges, *seen["args"][0], **seen["args"][1])
    torch.cuda.synchronize()
    assert torch.equal(arena.flat_param, arena_b.flat_param)
    assert torch.equal(arena.flat_mom, arena_b.flat_mom)


def test_sandwich_iteration_with_interpolation_and_a_second_step():
    from util_models import psp_head
    from gaia_seg_amd.core.synthetic import make_batch
    model = _tiny(psp_head(), seed=5)
    runner, arena = _sandwich_runner(model, kd=dict(T=4.0, distillation_weight=0.5, interpolation=True),
                                     random_member=False)
    before = arena.flat_param.clone()
    for it in range(2):
        out = runner.train_iter(make_batch(2, 64, 96, seed=it, device="cuda", border=2))
        assert torch.isfinite(out["loss"]).item()
        assert arena.grads_clean and not arena.flat_acc.any() and not arena.flat_grad.any()
    assert not torch.equal(before, arena.flat_param)
    assert runner.iter == 2


def test_sandwich_refuses_a_first_member_that_is_not_the_full_arch():
    from util_models import psp_head
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import SandwichHook
    from gaia_seg_amd.core.synthetic import make_batch
    model = _tiny(psp_head())
    runner, arena = _sandwich_runner(model)
    runner.hooks = [h for h in runner.hooks if not isinstance(h, SandwichHook)]
    runner.register_hook(SandwichHook(build_model_sampler(dict(type="concat", model_samplers=[
        dict(type="anchor", anchors=[_MINM, _MAXM])]))))
    with pytest.raises(AssertionError, match="full arch"):
        runner.train_iter(make_batch(2, 64, 96, device="cuda", border=2))


# ---- two ranks ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util_models import psp_head
    from gaia_seg_amd.core.synthetic import make_batch
    model = _tiny(psp_head(), seed=0)
    runner, arena = _sandwich_runner(model, random_member=False)
    # rank 1's sampler draws differently: only rank 0's draw may count
    runner.hooks[-1].sampler.seed(11 + 100 * rank)
    names = []
    for it in range(2):
        out = runner.train_iter(make_batch(2, 64, 96, seed=10 * it + rank, device="cuda", border=2))
        names.append(list(out["members"]) + [sorted(runner.arch_meta.items())])
    torch.cuda.synchronize()
    q.put((rank, names, arena.flat_param.double().sum().item(), arena.flat_param.abs().double().sum().item(),
           float(out["log_vars"]["loss"]), bool(arena.flat_acc.any())))
    dist.destroy_process_group()


def test_two_ranks_run_sandwich_iterations_in_lockstep():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    r0, r1 = out
    assert r0[1] == r1[1]                       # same members (incl. the random draw) on both ranks
    assert r0[2] == r1[2] and r0[3] == r1[3]    # bit-identical parameters after two iterations
    assert r0[4] == r1[4]                       # rank-averaged log vars
    assert not r0[5] and not r1[5]


def test_train_supernet_cli_with_inplace_distillation(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_supernet.py"),
           os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_inplace_distill.py"),
           "--work-dir", str(tmp_path), "--seed", "0", "--no-validate", "--max-iters", "2",
           "--cfg-options", "data.train.size=(64,128)", "log_config.interval=1",
           "checkpoint_config.interval=2"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stderr + res.stdout
    assert "Iter [2/2]" in out and "finished 2 iterations" in out
    for key in ("MAX.decode.loss_seg", "MIN.decode.loss_seg", "random0.aux.loss_seg", "random2.decode.acc_seg"):
        assert key in out, key
    ck = torch.load(os.path.join(str(tmp_path), "iter_2.pth"), map_location="cpu")
    assert set(ck) >= {"meta", "state_dict", "optimizer"}
    assert torch.isfinite(ck["state_dict"]["decode_head.conv_seg.weight"]).all()
