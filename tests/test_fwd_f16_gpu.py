"""The fp16 forward K loop (csrc/igemm_core.h packed_k_loop<PackF16>, gs_set_forward_precision(1)) at operator
level, its isolation from training, and a whole subnet's eval logits against an fp16-rounded oracle.

Operator witness: an fp64 convolution of the operands rounded to fp16 (round to nearest even; the
input after its fp32 BN + ReLU when in_affine is set).  The bound, 1e-6 of sum |a||b| per output,
is fp32-accumulation sized: the fp32 loops miss that witness by the fp16 rounding (~2^-11 per
operand), so these cases cannot pass without the f16 loop."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util_models import arch_meta, fcn_head, make_batch, make_pair, model_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-6

# n  h   w   ci   co   k  s  dil  in_affine  force_plan (bm, bn, splits)
CASES = [
    (1, 64, 128, 64, 256, 1, 1, 1, False, None),           # 1x1 (conv3 shape), four column tiles
    (1, 64, 128, 64, 256, 1, 1, 1, True, None),            # 1x1 on relu(bn(x)) (deferred conv3 input)
    (2, 64, 96, 64, 64, 3, 1, 1, False, None),             # 3x3, 64-wide tiles
    (2, 64, 96, 64, 64, 3, 1, 1, True, None),
    (2, 48, 80, 128, 128, 3, 1, 2, True, None),            # dilated 3x3
    (2, 64, 128, 128, 128, 3, 2, 1, False, None),          # strided 3x3 (a stage's first conv2)
    (2, 64, 128, 128, 128, 3, 2, 1, True, None),
    (1, 32, 64, 256, 256, 3, 1, 1, False, (64, 64, 3)),    # split-K, slabs combined in the launch
    (1, 32, 64, 256, 256, 3, 1, 1, True, (64, 64, 3)),
    (2, 64, 96, 48, 48, 3, 1, 1, True, None),              # MIN widths: 48-wide tiles
    (2, 40, 72, 80, 200, 3, 1, 1, False, (64, 48, 1)),     # ragged columns, Ci = 80 (odd K-step count)
]


def _affine(ci, g):
    # powers of two: (x - mean) * scale is exact, so fused or not, the loader rounds once (+ beta)
    scale = torch.pow(2.0, torch.randint(-1, 2, (ci,), generator=g).float())
    beta = torch.randn(ci, generator=g) * 0.2
    mean = torch.randn(ci, generator=g) * 0.2
    invstd = torch.ones(ci)
    return torch.stack([scale, beta, mean, invstd])          # [scale | beta | mean | invstd][C]


def _act(x, coeffs):
    """relu((x - mean) * scale + beta) in fp32, as the loader computes it."""
    scale, beta, mean = coeffs[0], coeffs[1], coeffs[2]
    return torch.relu((x - mean) * scale + beta)


def _run(hip_lib, lib, case, x, w_log, coeffs):
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    n, h, wd, ci, co, k, s, dil, aff, force = case
    d = lib.conv_desc(n, h, wd, ci, co, k, s, dil)
    xd = x.to(DEV).contiguous()
    wd_phys = w_log.permute(2, 3, 1, 0).contiguous().to(DEV)
    cd = coeffs.to(DEV).contiguous() if aff else None
    if aff:
        d.in_affine = cd.data_ptr()
    y = torch.full((n, d.Ho, d.Wo, co), float("nan"), device=DEV)
    hip_lib.gs_debug_set_stream_mode(0)
    if force:
        assert hip_lib.gs_debug_force_plan(*force) == 0
    try:
        need = hip_lib.gs_conv2d_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        lib.check(hip_lib.gs_conv2d_forward(ctypes.byref(d), xd.data_ptr(), wd_phys.data_ptr(), None, None,
                                            y.data_ptr(), ws.data_ptr(), need, current_stream_ptr()), "fwd")
    finally:
        hip_lib.gs_debug_force_plan(0, 0, 0)
        hip_lib.gs_debug_set_stream_mode(-1)
    torch.cuda.synchronize()
    rec = lib.DebugLaunch()
    assert hip_lib.gs_debug_last_conv_launch(ctypes.byref(rec)) == 0
    return y.cpu(), rec


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:8]) + ("_aff" if c[8] else ""))
def test_f16_forward_matches_rounded_fp64_witness(hip_lib, case):
    from gaia_seg_amd.hip import lib, ops
    n, h, wd, ci, co, k, s, dil, aff, force = case
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(n, h, wd, ci, generator=g)
    w_log = torch.randn(co, ci, k, k, generator=g) * 0.1
    coeffs = _affine(ci, g)
    a = _act(x, coeffs) if aff else x
    a16 = a.half().double().permute(0, 3, 1, 2)
    w16 = w_log.half().double()
    p = dil * (k // 2)
    want = F.conv2d(a16, w16, None, s, p, dil).permute(0, 2, 3, 1)
    mag = F.conv2d(a16.abs(), w16.abs(), None, s, p, dil).permute(0, 2, 3, 1)
    n0 = ctypes.c_int64()
    f0 = ctypes.c_double()
    hip_lib.gs_debug_f16_launches(ctypes.byref(n0), ctypes.byref(f0), 1)
    with ops.forward_precision("fp16"):
        assert hip_lib.gs_get_forward_precision() == 1
        got, rec = _run(hip_lib, lib, case, x, w_log, coeffs)
    assert hip_lib.gs_get_forward_precision() == 0
    assert rec.op == lib.OP_FORWARD and rec.kloop == lib.KLOOP_F16 and rec.in_affine == int(aff), rec.kloop
    if force:
        assert rec.splits == force[2]
    hip_lib.gs_debug_f16_launches(ctypes.byref(n0), ctypes.byref(f0), 1)
    assert n0.value == 1 and f0.value == pytest.approx(2.0 * n * rec_rows(got) * co * ci * k * k)
    err = float(((got.double() - want).abs() / mag.clamp_min(1e-30)).max())
    assert err < BOUND, (case, err)
    # the fp32 kernels (switch off) miss the same witness by the fp16 rounding
    got32, rec32 = _run(hip_lib, lib, case, x, w_log, coeffs)
    assert rec32.kloop != lib.KLOOP_F16
    err32 = float(((got32.double() - want).abs() / mag.clamp_min(1e-30)).max())
    assert err32 > 10 * BOUND, (case, err32)


def rec_rows(y):
    return y.shape[1] * y.shape[2]


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[7]], ids=["1x1", "3x3_aff", "splitk"])
def test_f16_lane_maps_exact_on_integer_data(hip_lib, case):
    """Small integers are exact in fp16 and their sums exact in fp32: any A / B lane-map or
    k-order error of the loop shows as a wrong integer."""
    from gaia_seg_amd.hip import lib, ops
    n, h, wd, ci, co, k, s, dil, aff, force = case
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-4, 5, (n, h, wd, ci), generator=g).float()
    w_log = torch.randint(-3, 4, (co, ci, k, k), generator=g).float()
    coeffs = torch.stack([torch.ones(ci), torch.randint(-2, 3, (ci,), generator=g).float(),
                          torch.randint(-2, 3, (ci,), generator=g).float(), torch.ones(ci)])
    a = torch.relu(x - coeffs[2] + coeffs[1]) if aff else x
    p = dil * (k // 2)
    want = F.conv2d(a.double().permute(0, 3, 1, 2), w_log.double(), None, s, p, dil).permute(0, 2, 3, 1)
    with ops.forward_precision("fp16"):
        got, rec = _run(hip_lib, lib, case, x, w_log, coeffs)
    assert rec.kloop == lib.KLOOP_F16
    assert torch.equal(got.double(), want)


# ---- isolation --------------------------------------------------------------------------------
def _metas(n, h, w):
    return [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False)
            for _ in range(n)]


def test_training_forward_refused_in_fp16_mode(hip_lib):
    from gaia_seg_amd.hip import ops
    prod, _ = make_pair(model_cfg(fcn_head(), aux=True))
    prod = prod.cuda().train()
    prod.manipulate_arch(arch_meta("sub"))
    img, gt = make_batch(2, 64, 96)
    with pytest.raises(RuntimeError, match="inference only"):
        with ops.forward_precision("fp16"):
            prod.train_step(dict(img=img.cuda(), img_metas=_metas(2, 64, 96), gt_semantic_seg=gt.cuda()), None)
    assert hip_lib.gs_get_forward_precision() == 0 and ops.FORWARD_PRECISION == 0
    with pytest.raises(KeyError):
        with ops.forward_precision("fp16"):
            assert hip_lib.gs_get_forward_precision() == 1
            raise KeyError("boom")
    assert hip_lib.gs_get_forward_precision() == 0 and ops.FORWARD_PRECISION == 0
    with pytest.raises(ValueError):
        ops.forward_precision("bf16")


def _train_once(prod, img, gt):
    out = prod.train_step(dict(img=img.cuda(), img_metas=_metas(*img.shape[:1], *img.shape[2:]),
                               gt_semantic_seg=gt.cuda()), None)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in prod.named_parameters() if p.grad is not None}
    bufs = {k: b.detach().cpu().clone() for k, b in prod.named_buffers()}
    return float(out["loss"]), {k: float(v) for k, v in out["log_vars"].items()}, grads, bufs


def test_training_after_fp16_eval_is_bit_identical(hip_lib):
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    img, gt = make_batch(2, 64, 96, seed=3)
    results = []
    for with_eval in (False, True):
        prod, _ = make_pair(model_cfg(fcn_head(), aux=True), seed=5)
        prod = prod.cuda()
        prod.manipulate_arch(arch_meta("sub"))
        if with_eval:
            wrap_fp16_model(prod)
            prod.eval()
            with torch.no_grad():
                labels = prod.simple_test_device(img.cuda(), _metas(2, 64, 96))
            assert labels.shape == (2, 64, 96)
            assert hip_lib.gs_get_forward_precision() == 0
            prod.fp16_enabled = False
        prod.train()
        results.append(_train_once(prod, img, gt))
    (l0, v0, g0, b0), (l1, v1, g1, b1) = results
    assert l0 == l1 and v0 == v1
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)


# ---- a whole subnet ----------------------------------------------------------------------------
def test_subnet_logits_fp16_against_rounded_oracle(hip_lib):
    """One subnet's eval logits in fp16 mode against the oracle's fp32 forward and against a witness:
    that forward with every conv's input and weight rounded to fp16 (the stem excepted: it stays
    fp32 in fp16 mode).  Relative rms, because a random-init network amplifies fp16-level
    perturbations too much for an absolute bound.

    Measured on one MI355X: fp32 vs oracle 6.2e-7, fp16 vs oracle 9.2e-4,
    witness vs oracle 9.2e-4, fp16 vs witness 5.4e-4.  The HIP fp16 logits move away from fp32 by
    the witness's amount (a kernel that ignores the switch stays at 6e-7 and fails), but they are
    not yet much closer to the witness than the witness is to fp32: that gap is open."""
    from gaia_seg_amd.hip import ops
    from oracle.model import OConv
    prod, orc = make_pair(model_cfg(fcn_head(), aux=False), seed=2)
    prod = prod.cuda().eval()
    orc.eval()
    meta = arch_meta("sub")
    prod.manipulate_arch(meta)
    orc.manipulate_arch(meta)
    img, _ = make_batch(2, 64, 96, seed=9)
    hip_lib.gs_debug_set_stream_mode(0)    # (the 1x1 streaming kernel stays fp32: keep it out)
    try:
        n0 = ctypes.c_int64()
        hip_lib.gs_debug_f16_launches(ctypes.byref(n0), None, 1)
        with torch.no_grad(), ops.forward_precision("fp16"):
            hip16 = prod.encode_decode(img.cuda(), _metas(2, 64, 96)).float().cpu()
        hip_lib.gs_debug_f16_launches(ctypes.byref(n0), None, 1)
        with torch.no_grad():
            hip32 = prod.encode_decode(img.cuda(), _metas(2, 64, 96)).float().cpu()
    finally:
        hip_lib.gs_debug_set_stream_mode(-1)
    assert n0.value == 26       # every conv of the subnet but the stem
    with torch.no_grad():
        plain = orc.encode_decode(img)
        hooks = []
        saved = {}
        for name, m in orc.named_modules():
            if isinstance(m, OConv) and m.in_channels != 3:
                saved[name] = m.weight.detach().clone()
                m.weight.copy_(m.weight.half().float())
                hooks.append(m.register_forward_pre_hook(lambda mod, inp: (inp[0].half().float(),)))
        try:
            witness = orc.encode_decode(img)
        finally:
            for h in hooks:
                h.remove()
            for name, m in orc.named_modules():
                if name in saved:
                    m.weight.copy_(saved[name])

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    e16, e_w, e_ref, e32 = rel(hip16, plain), rel(hip16, witness), rel(witness, plain), rel(hip32, plain)
    print("relative rms: fp16 vs oracle %.3e, fp16 vs witness %.3e, witness vs oracle %.3e, fp32 vs oracle "
          "%.3e" % (e16, e_w, e_ref, e32))
    assert e32 < 1e-5                           # the fp32 path is untouched
    assert e16 > 100 * e32                      # the switch reached the kernels
    assert 0.5 * e_ref < e16 < 2.0 * e_ref      # by as much as rounding the operands moves the oracle
    assert e_w < e_ref                          # and in the witness's direction
