"""gs_ce_*, gs_resize_argmax through the C-ABI (csrc/loss.hip) against float64, under the protocol of
tests/test_attention_gpu.py:

  * the logits are passed through the descriptor's strides in two layouts: NHWC with a channel pitch of
    Cls + 5 and NaN in the pad columns, and NCHW contiguous;
  * every output is pre-filled with a sentinel and followed by a sentinel tail; dlogits' pad columns
    Cls..ld_d-1 must be exactly 0.0, the tail untouched, no NaN anywhere;
  * workspaces are exactly the queried size, hold 0xFF (NaN), and sit in front of a 4 KiB guard: a corner sum
    of a tile that no workgroup wrote would reach dlogits as NaN;
  * every call runs twice and the two results are bit-identical (fixed summation order, no atomics);
  * the backward runs in three forms -- gs_ce_backward_ws with its workspace (the tile forms), with
    workspace = NULL, and gs_ce_backward (both the gather form: bit-identical to each other).

Bounds: 5e-5 in conftest.rel_err for lse, dlogits and the probabilities, 2e-5 * max(1, |ref|) for the loss --
this operator's bounds in tests/test_hip_ops_gpu.py; the correct-count and the argmax are exact.
tests/test_ce_loss.py checks on the CPU that float32 torch stays below 1e-5 on these inputs (measured at most
1.1e-6 dlogits, 4.0e-7 lse, 8.1e-7 softmax) and that no argmax is decided by less than 1e-4, and asserts the
launch each case of tests/util_ce.py reaches."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
import util_ce as U

pytestmark = pytest.mark.gpu
DEV = U.DEV
GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4


def fmt(errs):
    return {k: "%.2e" % v for k, v in errs.items()}


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_ce_forward(hip_lib, case):
    n = case.shape[0]
    numel = n * case.size[0] * case.size[1]
    scales = (0.4 / numel, 100.0 / numel)
    for weighted in (False, True):
        ref = U.ce_ref(case.name, weighted)
        for layout in U.LAYOUTS:
            op = U.Operands(case, layout, weighted)
            out, lse = U.run_forward(hip_lib, op)
            out_b, lse_b = U.run_forward(hip_lib, op)
            assert torch.equal(out, out_b) and torch.equal(lse, lse_b), "two runs differ"
            loss, count = float(out[0]), float(out[1])
            errs = {"loss": abs(loss - ref.loss) / max(1.0, abs(ref.loss)), "lse": rel_err(lse, ref.lse)}
            print(case.name, layout, "weighted" if weighted else "plain", fmt(errs), "count %d" % count)
            assert errs["loss"] < U.LOSS_TOL, "loss %r, reference %r" % (loss, ref.loss)
            assert count == ref.correct, "correct-count %r, reference %d" % (count, ref.correct)
            assert errs["lse"] < U.TOL
            if case.shape[1] == 1:
                assert loss == 0.0, "one class: the loss must be exactly 0.0"
            # lse is optional
            out_n, _ = U.run_forward(hip_lib, op, with_lse=False)
            assert torch.equal(out_n, out), "lse = NULL changed the result"
            # the scaled form: float32(out) * scale, rounded once, from gs_ce_forward's own output
            out2, lse2 = U.run_forward(hip_lib, op, scales=scales)
            out2_b, _ = U.run_forward(hip_lib, op, scales=scales)
            want = np.float32(out.numpy()) * np.array(scales, dtype=np.float32)
            assert want.dtype == np.float32
            assert out2.numpy().tobytes() == want.tobytes(), "scaled %r, float32(out) * scale %r" % (out2, want)
            assert torch.equal(out2, out2_b) and torch.equal(lse2, lse)


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_ce_backward_three_forms(hip_lib, case):
    worst = {}
    for variant in U.backward_variants(case):
        weighted, layout, ld_d, gi = variant
        gs = U.grad_scale_of(case, gi)
        ref = U.ce_ref(case.name, weighted)
        want = ref.dlogits * gs
        op = U.Operands(case, layout, weighted)
        _, lse = U.run_forward(hip_lib, op)
        lse_dev = lse.to(DEV)
        need = hip_lib.gs_ce_backward_workspace_bytes(op.db(), ld_d)
        assert (need == 0) == (case.route[0] == "gather"), "the workspace query is 0 exactly for the gather form"
        got = {}
        for form in U.FORMS:
            if form == "ws" and need == 0:
                continue
            got[form] = U.run_backward(hip_lib, op, lse_dev, form, ld_d, gs)
            again = U.run_backward(hip_lib, op, lse_dev, form, ld_d, gs)
            assert torch.equal(got[form], again), "%s: two runs differ" % form
        assert torch.equal(got["null"], got["direct"]), "workspace = NULL and gs_ce_backward run the same kernel"
        errs = {form: rel_err(g, want) for form, g in got.items()}
        print(case.name, "weighted" if weighted else "plain", layout, "ld_d %d" % ld_d, "grad_scale %.3g" % gs,
              fmt(errs))
        for form, g in got.items():
            if case.shape[1] == 1:
                assert not bool(g.any()), "%s: one class, every gradient must be exactly 0.0" % form
            assert errs[form] < U.TOL, "%s %s: rel_err %.3g" % (form, variant, errs[form])
            worst[form] = max(worst.get(form, 0.0), errs[form])
    print(case.name, "worst", fmt(worst))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_ce_label_prob(hip_lib, case):
    from gaia_seg_amd.hip import lib
    inp, ref = U.ce_inputs(case.name), U.ce_ref(case.name, False)
    valid = U.valid_mask(case, inp.labels)
    for layout in U.LAYOUTS:
        op = U.Operands(case, layout, False)
        runs = []
        for _ in range(2):
            prob = U.Out(op.numel)
            lib.check(hip_lib.gs_ce_label_prob(op.db(), op.logits.data_ptr(), op.labels.data_ptr(), prob.ptr(),
                                               U.stream()), "gs_ce_label_prob")
            runs.append(prob.get("prob").view_as(ref.prob))
        assert torch.equal(runs[0], runs[1]), "two runs differ"
        got = runs[0]
        err = rel_err(got[valid], ref.prob[valid])
        print(case.name, layout, "prob %.2e" % err, "%d invalid" % int((~valid).sum()))
        assert err < U.TOL
        assert bool((got[~valid] == 2.0).all()), "ignored and out-of-range labels must give exactly 2.0"


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_resize_argmax(hip_lib, case):
    from gaia_seg_amd.hip import lib
    ref = U.ce_ref(case.name, False)
    cls = case.shape[1]
    for layout in U.LAYOUTS:
        op = U.Operands(case, layout, False)
        for want_seg, want_probs in ((True, False), (False, True), (True, True)):
            runs = []
            for _ in range(2):
                seg = U.Out(op.numel, torch.int64, -7)
                probs = U.Out(op.numel * cls)
                lib.check(hip_lib.gs_resize_argmax(op.db(), op.logits.data_ptr(), seg.ptr() if want_seg else None,
                                                   probs.ptr() if want_probs else None, U.stream()),
                          "gs_resize_argmax")
                assert want_seg or seg.untouched()
                assert want_probs or probs.untouched()
                runs.append((seg.get("seg").view_as(ref.argmax) if want_seg else None,
                             probs.get("probs").view_as(ref.softmax) if want_probs else None))
            if want_seg:
                assert torch.equal(runs[0][0], runs[1][0])
                assert torch.equal(runs[0][0], ref.argmax), "argmax (the lowest index of a tied maximum)"
            if want_probs:
                got = runs[0][1]
                assert torch.equal(got, runs[1][1])
                err, row = rel_err(got, ref.softmax), float((got.double().sum(-1) - 1).abs().max())
                print(case.name, layout, "probs %.2e" % err, "row sums within %.2e" % row)
                assert err < U.TOL and row < 1e-5


def test_ce_argument_checks(hip_lib):
    """each documented error code; the outputs still hold the sentinel afterwards, and both workspace queries
    return 0 for a refused descriptor"""
    L, st = hip_lib, U.stream()
    case = U.CASES[0]
    n, cls, h, w = case.shape
    op = U.Operands(case, "nchw", True)
    numel = op.numel
    lse_in = torch.zeros(numel, device=DEV)
    outs = {"lse": U.Out(numel), "out": U.Out(2, torch.float64), "out2": U.Out(2), "prob": U.Out(numel),
            "dl": U.Out(n * h * w * cls), "seg": U.Out(numel, torch.int64, -7), "probs": U.Out(numel * cls)}
    need = L.gs_ce_workspace_bytes(op.db())
    need_b = L.gs_ce_backward_workspace_bytes(op.db(), cls)
    assert need > 0 and need_b > 0
    ws = torch.zeros(max(need, need_b) + 8, dtype=torch.uint8, device=DEV)
    lg, lb = op.logits.data_ptr(), op.labels.data_ptr()

    def ref_of(d):
        return ctypes.byref(d) if d is not None else None

    def fwd(d, logits=lg, labels=lb, out=outs["out"].ptr(), wsp=ws.data_ptr(), wsb=need):
        return L.gs_ce_forward(ref_of(d), logits, labels, op.pw_ptr(), op.cw_ptr(), outs["lse"].ptr(), out, wsp, wsb,
                               st)

    def fwd_scaled(d, logits=lg, labels=lb, out=outs["out2"].ptr(), wsp=ws.data_ptr(), wsb=need):
        return L.gs_ce_forward_scaled(ref_of(d), logits, labels, op.pw_ptr(), op.cw_ptr(), outs["lse"].ptr(), 0.5,
                                      0.5, out, wsp, wsb, st)

    def bwd(d, logits=lg, labels=lb, lse=lse_in.data_ptr(), dl=outs["dl"].ptr(), ld_d=cls):
        return L.gs_ce_backward(ref_of(d), logits, labels, op.pw_ptr(), op.cw_ptr(), lse, 1.0, dl, ld_d, st)

    def bwd_ws(d, logits=lg, labels=lb, lse=lse_in.data_ptr(), dl=outs["dl"].ptr(), ld_d=cls):
        return L.gs_ce_backward_ws(ref_of(d), logits, labels, op.pw_ptr(), op.cw_ptr(), lse, 1.0, dl, ld_d,
                                   ws.data_ptr(), need_b, st)

    def label_prob(d, logits=lg, labels=lb, prob=outs["prob"].ptr()):
        return L.gs_ce_label_prob(ref_of(d), logits, labels, prob, st)

    def argmax(d, logits=lg, seg=outs["seg"].ptr(), probs=outs["probs"].ptr()):
        return L.gs_resize_argmax(ref_of(d), logits, seg, probs, st)

    def desc(**kw):
        d = type(op.desc).from_buffer_copy(op.desc)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    good = desc()
    calls = (fwd, fwd_scaled, bwd, bwd_ws, label_prob, argmax)
    # GS_E_NULL
    assert all(f(None) == GS_E_NULL for f in calls)
    assert all(f(good, logits=None) == GS_E_NULL for f in calls)
    assert all(f(good, labels=None) == GS_E_NULL for f in (fwd, fwd_scaled, bwd, bwd_ws, label_prob))
    assert fwd(good, out=None) == GS_E_NULL and fwd_scaled(good, out=None) == GS_E_NULL
    assert fwd(good, wsp=None) == GS_E_NULL and fwd_scaled(good, wsp=None) == GS_E_NULL
    assert all(f(good, lse=None) == GS_E_NULL and f(good, dl=None) == GS_E_NULL for f in (bwd, bwd_ws))
    assert label_prob(good, prob=None) == GS_E_NULL
    assert argmax(good, seg=None, probs=None) == GS_E_NULL
    assert L.gs_ce_workspace_bytes(None) == 0 and L.gs_ce_backward_workspace_bytes(None, cls) == 0
    # GS_E_BADARG
    for field in ("N", "h", "w", "Cls", "H", "W"):
        for value in (0, -2):
            bad = desc(**{field: value})
            assert all(f(bad) == GS_E_BADARG for f in calls), "%s = %d" % (field, value)
            assert L.gs_ce_workspace_bytes(ctypes.byref(bad)) == 0
            assert L.gs_ce_backward_workspace_bytes(ctypes.byref(bad), cls) == 0
    assert bwd(good, ld_d=cls - 1) == GS_E_BADARG and bwd_ws(good, ld_d=cls - 1) == GS_E_BADARG
    assert L.gs_ce_backward_workspace_bytes(ctypes.byref(good), cls - 1) == 0
    # GS_E_WORKSPACE, GS_E_ALIGN
    assert fwd(good, wsb=need - 1) == GS_E_WORKSPACE and fwd_scaled(good, wsb=need - 1) == GS_E_WORKSPACE
    assert fwd(good, wsb=0) == GS_E_WORKSPACE
    assert fwd(good, wsp=ws.data_ptr() + 4) == GS_E_ALIGN and fwd_scaled(good, wsp=ws.data_ptr() + 4) == GS_E_ALIGN
    for name, o in outs.items():
        assert o.untouched(), "a refused call wrote to %s" % name


def _rowcls_defaults(hip_lib):
    """the row-tile cases' dlogits of the default instantiation, keyed like the child's runs"""
    res = {}
    for case in U.ROWTILE_CASES:
        for variant in U.backward_variants(case):
            weighted, layout, ld_d, gi = variant
            op = U.Operands(case, layout, weighted)
            _, lse = U.run_forward(hip_lib, op)
            res[U.variant_key(case, variant, "ws")] = U.run_backward(hip_lib, op, lse.to(DEV), "ws", ld_d,
                                                                     U.grad_scale_of(case, gi))
    return res


@pytest.mark.parametrize("rowcls", ["10", "4"])
def test_ce_backward_rowtile_instantiations(hip_lib, tmp_path, rowcls):
    """ce_bwd_rowtile_kernel<10> and <4>: GS_CE_ROWCLS is read once per process, so each runs in one fresh
    child process (tests/util_ce.py main) with the same float64 bound, guards and sentinels"""
    assert os.environ.get("GS_CE_ROWCLS") in (None, "", "5"), "this process must run the default instantiation"
    path = str(tmp_path / "defaults.pt")
    torch.save(_rowcls_defaults(hip_lib), path)
    env = dict(os.environ, GS_CE_ROWCLS=rowcls)
    res = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util_ce.py"),
                          path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, "GS_CE_ROWCLS=%s: exit %d\n%s" % (rowcls, res.returncode, res.stdout[-2000:])
    assert "GS_CE_ROWCLS=%s" % rowcls in res.stdout
    assert res.stdout.count("bit-identical") == len(U.ROWTILE_CASES)
