"""fp16 training on the MI355X: the f16 data-gradient K loop (csrc/igemm_core.h packed_k_loop<PackF16, ..., BFWD=false>,
gs_set_train_precision(1)) at operator level, and the training step with fp16 operands and a static
loss scale (core/runner.py Fp16ArenaOptimizerHook).

Operator witness: an fp64 transposed convolution of dy and W rounded to fp16 (round to nearest even).
The bound, 1e-6 of sum |dy||W| per output, is fp32-accumulation sized: the fp32 loops miss that
witness by the fp16 rounding (~2^-11 per operand), so these cases cannot pass without the f16 loop.
Every test that flips the switch restores it in finally."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from util_models import arch_meta, fcn_head, make_batch, model_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-6

# n  h    w    ci   co   k  s  dil ldx  force_plan (bm, bn, splits)
CASES = [
    (2, 63, 65, 512, 64, 1, 1, 1, 512, None),             # 1x1, ragged M tail
    (2, 64, 96, 64, 64, 3, 1, 1, 64, None),               # 3x3, 64-wide tiles
    (2, 48, 80, 128, 128, 3, 1, 2, 128, None),            # dilated 3x3
    (2, 64, 128, 128, 128, 3, 2, 1, 128, None),           # strided 3x3: four parity classes
    (2, 64, 128, 256, 64, 1, 2, 1, 256, None),            # strided 1x1: one class, three zero
    (1, 32, 64, 256, 256, 3, 1, 1, 256, (64, 64, 3)),     # split-K, slabs combined in the launch
    (2, 64, 96, 48, 48, 3, 1, 1, 48, None),               # MIN widths: 48-wide tiles
    (2, 40, 72, 200, 80, 3, 1, 1, 200, (64, 48, 1)),      # ragged columns (Ci = 200), Co = 80: odd K steps
    (2, 64, 64, 64, 144, 3, 1, 1, 112, None),             # pixel stride of dx wider than C
]


def _dgrad(hip_lib, lib, case, dy, w_log, train_mode):
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    n, h, wd, ci, co, k, s, dil, ldx, force = case
    d = lib.conv_desc(n, h, wd, ci, co, k, s, dil, ldx=ldx)
    w_phys = w_log.permute(2, 3, 1, 0).contiguous().to(DEV)
    dx = torch.full((n, h, wd, ldx), 7.0, device=DEV)
    hip_lib.gs_debug_set_stream_mode(0)
    if force:
        assert hip_lib.gs_debug_force_plan(*force) == 0
    assert hip_lib.gs_set_train_precision(train_mode) == 0
    try:
        need = hip_lib.gs_conv2d_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        q = lib.DebugLaunch()
        assert hip_lib.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_DGRAD, ctypes.byref(q)) == 0
        lib.check(hip_lib.gs_conv2d_dgrad(ctypes.byref(d), dy.to(DEV).contiguous().data_ptr(),
                                          w_phys.data_ptr(), dx.data_ptr(), 0, ws.data_ptr(), need,
                                          current_stream_ptr()), "dgrad")
    finally:
        hip_lib.gs_set_train_precision(0)
        hip_lib.gs_debug_force_plan(0, 0, 0)
        hip_lib.gs_debug_set_stream_mode(-1)
    torch.cuda.synchronize()
    rec = lib.DebugLaunch()
    assert hip_lib.gs_debug_last_conv_launch(ctypes.byref(rec)) == 0
    # (the query describes parity class (0, 0) of a strided dgrad, the record its last class)
    if s == 1 or train_mode:
        assert (q.kloop, q.bm, q.bn) == (rec.kloop, rec.bm, rec.bn)
    out = dx.cpu()
    if ldx > ci:
        assert bool((out[..., ci:] == 7.0).all())       # columns beyond the slice untouched
    return out[..., :ci], rec


def _witness(case, dy, w_log):
    n, h, wd, ci, co, k, s, dil, ldx, force = case
    p = dil * (k // 2)
    dy16 = dy.half().double().permute(0, 3, 1, 2)
    w16 = w_log.half().double()
    want = torch.nn.grad.conv2d_input((n, ci, h, wd), w16, dy16, s, p, dil).permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_input((n, ci, h, wd), w16.abs(), dy16.abs(), s, p, dil).permute(0, 2, 3, 1)
    return want, mag


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_f16_dgrad_matches_rounded_fp64_witness(hip_lib, case):
    from gaia_seg_amd.hip import lib
    n, h, wd, ci, co, k, s, dil, ldx, force = case
    g = torch.Generator().manual_seed(4321)
    p = dil * (k // 2)
    ho, wo = (h + 2 * p - dil * (k - 1) - 1) // s + 1, (wd + 2 * p - dil * (k - 1) - 1) // s + 1
    dy = torch.randn(n, ho, wo, co, generator=g)
    w_log = torch.randn(co, ci, k, k, generator=g) * 0.1
    want, mag = _witness(case, dy, w_log)
    nb = (ctypes.c_int64 * 2)()
    fb = (ctypes.c_double * 2)()
    hip_lib.gs_debug_f16_launches_by_op(nb, fb, 1)
    got, rec = _dgrad(hip_lib, lib, case, dy, w_log, 1)
    assert hip_lib.gs_get_train_precision() == 0
    assert rec.op == lib.OP_DGRAD and rec.kloop == lib.KLOOP_F16, rec.kloop
    assert rec.bm == 64 and rec.bn in (64, 48)
    if force:
        assert rec.splits == force[2]
    hip_lib.gs_debug_f16_launches_by_op(nb, fb, 1)
    assert nb[lib.OP_FORWARD] == 0 and nb[lib.OP_DGRAD] >= 1
    err = float(((got.double() - want).abs() / mag.clamp_min(1e-30)).max())
    assert err < BOUND, (case, err)
    # the fp32 loops (switch off) miss the same witness by the fp16 rounding
    got32, rec32 = _dgrad(hip_lib, lib, case, dy, w_log, 0)
    assert rec32.kloop != lib.KLOOP_F16
    err32 = float(((got32.double() - want).abs() / mag.clamp_min(1e-30)).max())
    assert err32 > 10 * BOUND, (case, err32)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5], CASES[6]], ids=["1x1", "strided", "splitk", "bn48"])
def test_f16_dgrad_lane_maps_exact_on_integer_data(hip_lib, case):
    """Small integers are exact in fp16 and their sums exact in fp32: any A / B lane-map or k-order
    error of the data-gradient loop shows as a wrong integer."""
    from gaia_seg_amd.hip import lib
    n, h, wd, ci, co, k, s, dil, ldx, force = case
    g = torch.Generator().manual_seed(11)
    p = dil * (k // 2)
    ho, wo = (h + 2 * p - dil * (k - 1) - 1) // s + 1, (wd + 2 * p - dil * (k - 1) - 1) // s + 1
    dy = torch.randint(-4, 5, (n, ho, wo, co), generator=g).float()
    w_log = torch.randint(-3, 4, (co, ci, k, k), generator=g).float()
    want = torch.nn.grad.conv2d_input((n, ci, h, wd), w_log.double(), dy.double().permute(0, 3, 1, 2),
                                      s, p, dil).permute(0, 2, 3, 1)
    got, rec = _dgrad(hip_lib, lib, case, dy, w_log, 1)
    assert rec.kloop == lib.KLOOP_F16
    assert torch.equal(got.double(), want)


# ---- the training step -----------------------------------------------------------------------
def _metas(n, h, w):
    return [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False)
            for _ in range(n)]


def _runner(seed=5, arch="sub", fp16=False, loss_scale=1.0, lr=0.02):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    from gaia_seg_amd.models import build_segmentor
    from util_models import randomize
    model = build_segmentor(copy.deepcopy(model_cfg(fcn_head(), aux=True)))
    randomize(model, seed)
    model = model.cuda().train()
    model.manipulate_arch(arch_meta(arch))
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=lr,
                             momentum=0.9, weight_decay=1e-4, max_iters=100)
    runner.set_arch(None)
    runner.register_hook(ArenaOptimizerHook())
    runner.call_hook("before_run")
    runner.train_precision = "fp16" if fp16 else "fp32"
    runner.loss_scale = loss_scale
    return runner


def _batch(seed=3, n=2, h=64, w=96):
    img, gt = make_batch(n, h, w, seed=seed)
    return dict(img=img.cuda(), img_metas=_metas(n, h, w), gt_semantic_seg=gt.cuda())


def _state(runner):
    torch.cuda.synchronize()
    a = runner.arena
    bufs = {k: b.detach().cpu().clone() for k, b in runner.model.named_buffers()}
    return a.flat_param.detach().cpu().clone(), a.flat_mom.detach().cpu().clone(), bufs


def _counts(hip_lib, lib):
    c = (ctypes.c_int64 * (3 * lib.KLOOP_COUNT * 3))()
    hip_lib.gs_debug_conv_launch_counts(c, 1)
    nb = (ctypes.c_int64 * 2)()
    hip_lib.gs_debug_f16_launches_by_op(nb, None, 1)
    per = {(o, k): sum(c[(o * lib.KLOOP_COUNT + k) * 3 + m] for m in range(3))
           for o in range(3) for k in range(lib.KLOOP_COUNT)}
    return per, (nb[0], nb[1])


@pytest.mark.parametrize("arch", ["sub", "max"])
def test_fp16_step_launch_accounting(hip_lib, arch):
    """One fp16 step puts every forward and data-gradient launch that ran on a fast fp32 / bf16x3 loop
    in the fp32 step on the f16 loop -- nothing else moves: the stem and streaming / generic launches
    and every weight gradient are counted exactly as in fp32."""
    from gaia_seg_amd.hip import lib
    fast = (lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS, lib.KLOOP_BF16X3)
    batch = _batch()
    res = {}
    for fp16 in (False, True):
        r = _runner(arch=arch, fp16=fp16, loss_scale=512.0 if fp16 else 1.0)
        r.train_iter(batch)                    # (first step: lazily created handles)
        torch.cuda.synchronize()
        _counts(hip_lib, lib)
        r.train_iter(batch)
        torch.cuda.synchronize()
        res[fp16] = _counts(hip_lib, lib)
        assert hip_lib.gs_get_train_precision() == 0
    (c32, f32), (c16, f16) = res[False], res[True]
    assert f32 == (0, 0)
    for op, f16n in ((lib.OP_FORWARD, f16[0]), (lib.OP_DGRAD, f16[1])):
        moved = sum(c32[(op, k)] for k in fast)
        assert moved > 0 and f16n == moved, (op, f16n, moved)
        assert all(c16[(op, k)] == 0 for k in fast), (op, c16)
        for k in (lib.KLOOP_GENERIC, lib.KLOOP_STREAM):
            assert c16[(op, k)] == c32[(op, k)], (op, k)
    assert all(c16[(lib.OP_WGRAD, k)] == c32[(lib.OP_WGRAD, k)] for k in range(lib.KLOOP_COUNT))


def test_static_loss_scale_is_exact_with_fp32_operands(hip_lib):
    """fp32 operands with S = 512: parameters, momentum and BatchNorm buffers over 3 steps are
    bitwise those of S = 1 (a power of two scales every rounding exactly)."""
    batch = _batch()
    out = []
    for s in (1.0, 512.0):
        r = _runner(loss_scale=s)
        logs = []
        for _ in range(3):
            logs.append(float(r.train_iter(batch)["log_vars"]["loss"]))
        out.append((_state(r), logs))
    (p1, m1, b1), l1 = out[0]
    (p2, m2, b2), l2 = out[1]
    assert l1 == l2                              # log_vars report the unscaled loss
    assert torch.equal(p1, p2) and torch.equal(m1, m2)
    assert all(torch.equal(b1[k], b2[k]) for k in b1)


class _F16Conv(torch.autograd.Function):
    """A conv of the witness: forward on x and W rounded to fp16; dx from round16(S * dy) and
    round16(W), divided by S (only where the HIP data gradient takes the f16 loop: round_dx); dW on the
    unrounded x and dy, as the HIP weight gradient (fp32 operands)."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, dilation, scale, round_dx):
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, padding, dilation, scale, round_dx)
        return F.conv2d(x.half().to(x.dtype), w.half().to(w.dtype), None, stride, padding, dilation)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, dilation, scale, round_dx = ctx.conf
        if round_dx:
            g16 = (gy * scale).half().to(gy.dtype)
            dx = torch.nn.grad.conv2d_input(x.shape, w.half().to(w.dtype), g16, stride, padding,
                                            dilation) / scale
        else:
            dx = torch.nn.grad.conv2d_input(x.shape, w, gy, stride, padding, dilation)
        dw = torch.nn.grad.conv2d_weight(x, w.shape, gy, stride, padding, dilation)
        return dx, dw, None, None, None, None, None


def _witness_conv(scale):
    def dyn_conv2d(x, weight, bias, width, stride=1, padding=0, dilation=1):
        w = weight[:width, :x.size(1)]
        if x.size(1) == 3:            # the stem stays fp32
            y = F.conv2d(x, w, None, stride, padding, dilation)
        else:
            # the fast data-gradient kernel (hence the f16 loop): dy channels a multiple of 16, 1x1 / 3x3
            round_dx = width % 16 == 0 and w.shape[-1] in (1, 3)
            y = _F16Conv.apply(x, w, stride, padding, dilation, scale, round_dx)
        return y if bias is None else y + bias[:width].view(1, -1, 1, 1)
    return dyn_conv2d


def _hip_step_scaled(prod, img, gt, scale):
    """tests/parity.py hip_train_step with backward seeded by the loss scale."""
    from gaia_seg_amd.hip import ops
    n, _, h, w = img.shape
    ops.RELU_TRACE, ops.POOL_TRACE = [], []
    try:
        out = prod.train_step(dict(img=img.cuda(), img_metas=_metas(n, h, w), gt_semantic_seg=gt.cuda()),
                              None)
        trace, ptrace = ops.RELU_TRACE, ops.POOL_TRACE
    finally:
        ops.RELU_TRACE = ops.POOL_TRACE = None
    out["loss"].backward(gradient=torch.full_like(out["loss"], scale))
    torch.cuda.synchronize()
    names = {id(p): k for k, p in prod.named_parameters()}
    masks = {names[id(w_)][:-len(".weight")]: m.permute(0, 3, 1, 2).cpu() for w_, m in trace}
    pools = {"backbone.maxpool": ptrace[0].permute(0, 3, 1, 2).cpu()} if ptrace else {}
    return out, masks, pools


def _grad_vec(model, names, scale=1.0):
    p = dict(model.named_parameters())
    return torch.cat([p[k].grad.detach().double().cpu().flatten() for k in names]) / scale


def test_fp16_step_gradients_against_rounded_witness(hip_lib, monkeypatch):
    """One fp16 step's gradients (S = 512) against the fp64 oracle on the step's own ReLU / pool
    branches (tests/parity.py protocol), plain and as the witness (_F16Conv on every non-stem conv).
    The fused BatchNorm-backward epilogue runs on f16 data gradients in this step (asserted), so its
    dx and sums are inside the comparison.  Relative rms over all parameter gradients; bounds measured
    on one MI355X and stated in DESIGN.md section 17."""
    import gaia_seg_amd.hip.ops as ops
    from gaia_seg_amd.hip import lib
    from oracle import ops as O
    from parity import oracle_step
    from util_models import make_pair
    scale = 512.0
    prod, orc = make_pair(model_cfg(fcn_head(), aux=True), seed=5)
    prod = prod.cuda().train()
    orc.train()
    prod.manipulate_arch(arch_meta("sub"))
    orc.manipulate_arch(arch_meta("sub"))
    img, gt = make_batch(2, 64, 96, seed=3)
    hip_lib.gs_debug_set_stream_mode(0)    # (the 1x1 streaming kernel stays fp32: keep it out)
    fused0 = ops.BNBWD_FUSED_COUNT
    try:
        _counts(hip_lib, lib)
        with ops.train_precision("fp16"):
            out, masks, pools = _hip_step_scaled(prod, img, gt, scale)
        c16, f16 = _counts(hip_lib, lib)
    finally:
        hip_lib.gs_debug_set_stream_mode(-1)
    assert ops.BNBWD_FUSED_COUNT > fused0                 # BN backward fused into dgrad epilogues ...
    fast = (lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS, lib.KLOOP_BF16X3)
    assert f16[1] > 0 and all(c16[(lib.OP_DGRAD, k)] == 0 for k in fast), c16   # ... of f16 launches
    names = sorted(k for k, p in prod.named_parameters() if p.grad is not None and bool(p.grad.any()))
    hip16 = _grad_vec(prod, names, scale)
    bufs0 = {k: v.detach().clone() for k, v in orc.named_buffers()}
    oracle_step(orc, img, gt, masks, pools)
    exact = _grad_vec(orc, names)
    with torch.no_grad():
        for k, b in orc.named_buffers():
            b.copy_(bufs0[k].to(b.dtype))
    monkeypatch.setattr(O, "dyn_conv2d", _witness_conv(scale))
    oracle_step(orc, img, gt, masks, pools)
    witness = _grad_vec(orc, names)

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    e_w, e_ref, e_h = rel(hip16, witness), rel(witness, exact), rel(hip16, exact)
    print("gradient relative rms: fp16 vs witness %.3e, witness vs oracle %.3e, fp16 vs oracle %.3e"
          % (e_w, e_ref, e_h))
    # measured: fp16 vs witness 5.0e-3, witness vs oracle 1.6e-2, fp16 vs oracle 1.5e-2
    assert e_h > 1e-3                         # the switch reached the kernels
    assert e_w < 0.5 * e_ref, (e_w, e_ref)    # the gap is the operands' rounding ...
    assert e_w < 1e-2, e_w                    # ... up to accumulation-order noise


def test_fp16_fused_bn_backward_matches_unfused(hip_lib, monkeypatch):
    """The fused BatchNorm-backward epilogue (bn_bwd_mode) on the f16 loop against the separate
    BatchNorm-backward pass after a plain f16 data gradient: the same fp16 step, fused and unfused.
    The two sum in different orders; a difference of an fp32 ulp moves some of the next layer's fp16
    roundings by one fp16 step, so they agree to 1.9e-4 (measured), not to fp32 rounding -- a wrong
    epilogue would be O(1)."""
    import gaia_seg_amd.hip.ops as ops
    from util_models import make_pair
    batch = _batch()
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(ops, "BNBWD_FUSE", fuse)
        prod, _ = make_pair(model_cfg(fcn_head(), aux=True), seed=5)
        prod = prod.cuda().train()
        prod.manipulate_arch(arch_meta("sub"))
        n0 = ops.BNBWD_FUSED_COUNT
        with ops.train_precision("fp16"):
            out = prod.train_step(batch, None)
            out["loss"].backward(gradient=torch.full_like(out["loss"], 512.0))
        torch.cuda.synchronize()
        assert (ops.BNBWD_FUSED_COUNT > n0) == fuse
        names = sorted(k for k, p in prod.named_parameters() if p.grad is not None)
        res[fuse] = _grad_vec(prod, names, 512.0)
    err = float((res[True] - res[False]).norm() / res[False].norm())
    print("fused vs unfused BN backward, fp16 step: relative rms %.3e" % err)
    assert err < 5e-4, err


def test_fp16_short_convergence(hip_lib):
    """40 steps on a fixed learnable batch, fp16 static 512 against fp32: both losses fall, and the
    final losses agree closely."""
    n, h, w = 2, 64, 96
    torch.manual_seed(0)
    img = torch.randn(n, 3, h, w)
    sm = torch.nn.functional.avg_pool2d(img[:, :1], 9, 1, 4)
    gt = ((sm - sm.min()) / (sm.max() - sm.min() + 1e-6) * 5.999).long()
    batch = dict(img=img.cuda(), img_metas=_metas(n, h, w), gt_semantic_seg=gt.cuda())
    final = {}
    for fp16 in (False, True):
        r = _runner(fp16=fp16, loss_scale=512.0 if fp16 else 1.0)
        losses = [float(r.train_iter(batch)["log_vars"]["decode.loss_seg"]) for _ in range(40)]
        assert all(l == l for l in losses)
        assert losses[-1] < 0.5 * losses[0], losses[::10]
        final[fp16] = losses[-1]
    print("final decode loss fp32 %.5f fp16 %.5f" % (final[False], final[True]))
    # (measured 1.23699 fp32 vs 1.23800 fp16, 0.08 % apart after 40 steps)
    assert abs(final[True] - final[False]) < 0.02 * final[False], final


def test_graph_replay_equals_eager_in_fp16(hip_lib):
    """A captured fp16 step replayed equals the eager fp16 step bit for bit."""
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import ManipulateArchHook
    batch = _batch()
    states = []
    for graphs in (False, True):
        r = _runner(fp16=True, loss_scale=512.0)
        r.graphs_enabled = graphs
        sampler = build_model_sampler(dict(type="anchor", anchors=[
            {"name": "sub", "arch.backbone.stem.width": 16, "arch.backbone.body.width": [16, 48, 64, 96],
             "arch.backbone.body.depth": [1, 2, 2, 1]}]))
        r.register_hook(ManipulateArchHook(sampler))
        for _ in range(4):
            r.train_iter(batch)
        if graphs:
            assert r.graph_stats["captured"] == 1 and r.graph_stats["replayed"] >= 2, r.graph_stats
            assert any(k[-2:] == ("fp16", 512.0) for k in r._graphs)
        states.append(_state(r))
    assert hip_lib.gs_get_train_precision() == 0
    (p0, m0, b0), (p1, m1, b1) = states
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)


def test_fp16_isolation(hip_lib):
    """After an fp16 run -- returned, or raised mid-step -- the library is back in fp32 mode and an
    fp32 step is bit-identical to one in a run that never used fp16."""
    batch = _batch()
    states = []
    for used_fp16 in (False, True):
        if used_fp16:
            r16 = _runner(fp16=True, loss_scale=512.0)
            r16.train_iter(batch)
            assert hip_lib.gs_get_train_precision() == 0 and hip_lib.gs_get_forward_precision() == 0
            with pytest.raises(Exception):
                r16.train_iter(dict(batch, gt_semantic_seg=None))   # raises inside the fp16 step
            assert hip_lib.gs_get_train_precision() == 0
            torch.cuda.synchronize()
        r = _runner(seed=9)
        r.train_iter(batch)
        states.append(_state(r))
    (p0, m0, b0), (p1, m1, b1) = states
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)


def test_fp16_hook_checkpoint_meta_and_resume(hip_lib, tmp_path):
    """Fp16OptimizerHook: before_run turns fp16 on, wraps the model for fp16 eval and restores a
    scaler state from runner.meta; the checkpoint carries meta.fp16.loss_scaler (mmcv's keys) and
    resume() hands it back."""
    from gaia_seg_amd.apis.train import optimizer_hook
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.core.runner import CheckpointHook
    batch = _batch()
    r = _runner()
    r.hooks = [h for h in r.hooks if type(h).__name__ != "ArenaOptimizerHook"]
    r.register_hook(optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=256.)))
    r.register_hook(CheckpointHook(interval=2, out_dir=str(tmp_path)))
    r.call_hook("before_run")
    assert r.train_precision == "fp16" and r.loss_scale == 256.0 and r.model.fp16_enabled
    nb = (ctypes.c_int64 * 2)()
    hip_lib.gs_debug_f16_launches_by_op(None, None, 1)
    for _ in range(2):
        r.train_iter(batch)
    torch.cuda.synchronize()
    hip_lib.gs_debug_f16_launches_by_op(nb, None, 1)
    assert nb[0] > 0 and nb[1] > 0
    assert hip_lib.gs_get_train_precision() == 0
    ck = torch.load(os.path.join(str(tmp_path), "iter_2.pth"), map_location="cpu")
    ls = ck["meta"]["fp16"]["loss_scaler"]
    assert set(ls) == {"cur_scale", "cur_iter", "mode", "last_overflow_iter", "scale_factor",
                       "scale_window"} and ls["cur_scale"] == 256.0 and ls["mode"] == "static"
    # resume into a fresh runner whose hook was configured with another scale: the checkpoint wins
    ls2 = dict(ls, cur_scale=128.0)
    path = os.path.join(str(tmp_path), "edited.pth")
    save_checkpoint(r.model, path, optimizer=r.arena, meta=dict(iter=2, fp16=dict(loss_scaler=ls2)))
    r2 = _runner()
    r2.hooks = [h for h in r2.hooks if type(h).__name__ != "ArenaOptimizerHook"]
    r2.register_hook(optimizer_hook(dict(type="Fp16OptimizerHook", loss_scale=512.)))
    r2.resume(path)
    r2.call_hook("before_run")
    assert r2.iter == 2 and r2.loss_scale == 128.0 and r2.meta["fp16"]["loss_scaler"] == ls2


def test_train_supernet_cli_fp16_and_resume(tmp_path):
    """tools/train_supernet.py with the fp16 config on synthetic data: the log shows the loss scale,
    the checkpoint carries meta.fp16.loss_scaler, and --resume-from continues from it."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "tools", "train_supernet.py"),
            os.path.join(root, "configs", "supernet", "fcn_ar50to101v2_fp16.py"),
            "--work-dir", str(tmp_path), "--seed", "0", "--no-validate"]
    opts = ["--cfg-options", "data.train.size=(128,256)", "log_config.interval=1",
            "checkpoint_config.interval=2"]
    res = subprocess.run(base + ["--max-iters", "2"] + opts, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stderr + res.stdout
    assert "Iter [2/2]" in out and "loss_scale: 512" in out, out[-2000:]
    ck = torch.load(os.path.join(str(tmp_path), "iter_2.pth"), map_location="cpu")
    assert ck["meta"]["fp16"]["loss_scaler"]["cur_scale"] == 512.0
    assert ck["meta"]["fp16"]["loss_scaler"]["mode"] == "static"
    res = subprocess.run(base + ["--max-iters", "3", "--resume-from", os.path.join(str(tmp_path), "iter_2.pth")]
                         + opts, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = res.stderr + res.stdout
    assert "Iter [3/3]" in out and "Iter [1/3]" not in out and "loss_scale: 512" in out, out[-2000:]
