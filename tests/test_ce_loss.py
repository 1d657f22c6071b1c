"""The fused resize + cross-entropy operator without a GPU: the route every case of tests/util_ce.py takes
through gs_ce_backward_ws (from the host predicates alone, and through gs_ce_backward_workspace_bytes), the
workspace queries' refusals, and the conditioning of the GPU tests' inputs -- float32 torch stays a factor
of five inside the GPU bounds and no argmax is decided by less than 1e-4, so the bounds of
tests/test_ce_loss_gpu.py are statements about the kernels and not about the data."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_ce as U


def desc_of(case, **kw):
    from gaia_seg_amd.hip import lib
    n, cls, h, w = case.shape
    d = lib.CeDesc()
    d.N, d.h, d.w, d.Cls = n, h, w, cls
    d.H, d.W = case.size
    d.l_sn, d.l_sh, d.l_sw, d.l_sc = h * w * cls, w * cls, cls, 1
    d.ignore_index, d.align_corners = case.ignore, int(case.align)
    for key, val in kw.items():
        setattr(d, key, val)
    return d


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_case_takes_the_route_its_row_names(hip_lib, case):
    n, cls, h, w = case.shape
    assert U.route(case.shape, case.size, case.align) == case.route
    for ld_d in (cls, U.round_up(cls, 4) + 4):
        need = hip_lib.gs_ce_backward_workspace_bytes(ctypes.byref(desc_of(case)), ld_d)
        assert need == U.backward_workspace_bytes(case.shape, case.size, case.align, ld_d)
        assert (need == 0) == (case.route[0] == "gather")


def test_the_table_reaches_every_launch():
    by_name = {c.name: c for c in U.CASES}
    routes = [c.route for c in U.CASES]
    assert {(p, t) for p, t, _ in routes if p == "pow2"} == {("pow2", 64), ("pow2", 128), ("pow2", 256)}
    assert {g for _, _, g in routes} == {64, 128, 256}                 # gs_ce_backward runs on every case
    assert {t for p, t, _ in routes if p == "gather"} == {64, 256}    # the three gather-only cases
    assert [c.name for c in U.CASES if c.route[0] == "gather"] == ["gather-big", "gather-down", "gather-1x1-align"]
    assert len(U.ROWTILE_CASES) >= 6
    # mixed scale, 512 pixels per tile
    assert U.pow2_scales(*by_name["pow2-16x32"][1:4]) == (16, 32)
    # h = w = 1 and a second class pass of one class
    c = by_name["pow2-32x32-h1w1"]
    assert c.shape[2:] == (1, 1) and c.shape[1] == U.TCH + 1
    assert by_name["pow2-2x2-cls20"].shape[1] == U.TCH and by_name["rowtile-cls1"].shape[1] == 1
    assert by_name["gather-big"].shape[1] == U.CCH + 1
    # exactly on the row-tile threshold; 12 tiles leave 4 of the 16 row groups of the workgroup dead
    c = by_name["rowtile-64px-dead"]
    (n, cls, h, w), (hh, ww) = c.shape, c.size
    assert hh * ww == 64 * h * w and n * (h + 1) * (w + 1) % 16 == 12 and cls > 2 * U.TCH
    assert not U.rowtile_ok(c.shape, (hh, ww + 1))
    # about 38 pixels per non-empty tile: three passes of a 16-lane row
    c = by_name["rowtile-38px"]
    assert 32 < c.size[0] * c.size[1] / (c.shape[2] * c.shape[3]) <= 48
    # h == 1 with align_corners: the source scale along H is 0
    c = by_name["rowtile-align-h1"]
    assert c.align and c.shape[2] == 1
    # one output row and column with align_corners: scale == 0 in dst_range
    c = by_name["gather-1x1-align"]
    assert c.align and c.size == (1, 1)
    assert by_name["gather-down"].size[0] < by_name["gather-down"].shape[2]
    assert 0 <= by_name["ignore-in-range"].ignore < by_name["ignore-in-range"].shape[1]
    assert by_name["ignore-minus100"].ignore == -100
    assert max(c.size[0] * c.size[1] for c in U.CASES) <= 2048   # label pixels per image: the tests stay quick


BAD_FIELDS = [(f, v) for f in ("N", "h", "w", "Cls", "H", "W") for v in (0, -3)]


@pytest.mark.parametrize("field,value", BAD_FIELDS, ids=["%s=%d" % fv for fv in BAD_FIELDS])
def test_workspace_queries_return_zero_for_a_refused_descriptor(hip_lib, field, value):
    """h == 0 or w == 0 used to divide by zero on the host, N < 0 to return a huge size"""
    for case in (U.CASES[0], U.CASES[4]):
        cls = case.shape[1]
        assert hip_lib.gs_ce_backward_workspace_bytes(ctypes.byref(desc_of(case)), cls) > 0
        bad = desc_of(case, **{field: value})
        assert hip_lib.gs_ce_workspace_bytes(ctypes.byref(bad)) == 0
        assert hip_lib.gs_ce_backward_workspace_bytes(ctypes.byref(bad), max(cls, 32)) == 0


def test_workspace_queries_null_descriptor_and_short_pitch(hip_lib):
    assert hip_lib.gs_ce_workspace_bytes(None) == 0
    assert hip_lib.gs_ce_backward_workspace_bytes(None, 32) == 0
    for case in (U.CASES[0], U.CASES[4]):
        cls = case.shape[1]
        for ld_d in (cls - 1, 0, -4):
            assert hip_lib.gs_ce_backward_workspace_bytes(ctypes.byref(desc_of(case)), ld_d) == 0


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_inputs_are_well_conditioned(case):
    """float32 torch with the same formula stays below 1e-5 against float64 (a fifth of the GPU bound), and
    every pixel's top-2 gap is at least 1e-4, so the argmax and the correct-count compare exactly"""
    inp = U.ce_inputs(case.name)
    for weighted in (False, True):
        ref = U.ce_ref(case.name, weighted)
        f32 = U.ce_formula(case, inp, weighted, torch.float32)
        errs = {"dlogits": rel_err(f32.dlogits, ref.dlogits), "lse": rel_err(f32.lse, ref.lse),
                "prob": rel_err(f32.prob, ref.prob), "softmax": rel_err(f32.softmax, ref.softmax),
                "loss": abs(f32.loss - ref.loss) / max(abs(ref.loss), 1e-30)}
        print(case.name, "weighted" if weighted else "plain", {k: "%.2e" % v for k, v in errs.items()},
              "gap %.2e" % ref.gap)
        if case.shape[1] == 1:
            assert ref.loss == 0.0 and f32.loss == 0.0
            assert not bool(ref.dlogits.any()) and not bool(f32.dlogits.any())
            errs["loss"] = errs["dlogits"] = 0.0
        else:
            assert bool(ref.dlogits.any())
        for what, e in errs.items():
            assert e < 1e-5, "%s %s: %.3g" % (case.name, what, e)
        assert ref.gap >= 1e-4, "%s: top-2 gap %.3g, choose another seed" % (case.name, ref.gap)
        assert torch.equal(f32.argmax, ref.argmax) and f32.correct == ref.correct


def test_inputs_hold_what_the_gpu_tests_rely_on():
    for case in U.CASES:
        inp = U.ce_inputs(case.name)
        cls = case.shape[1]
        valid = U.valid_mask(case, inp.labels)
        if case.size == (1, 1):
            assert bool(valid.all())
            continue
        assert bool((inp.labels[:, 0] == case.ignore).all())
        assert sorted(int(inp.labels[p]) for p in inp.bad_pixels) == [-1, cls, 1 << 40]
        assert not bool(valid[:, 0].any()) and all(not bool(valid[p]) for p in inp.bad_pixels)
        assert int(valid.sum()) >= 4
        assert 0 < int(inp.pixel_weight.sum()) < inp.pixel_weight.numel()
        ref = U.ce_ref(case.name, False)
        assert bool((ref.prob[~valid] == 2.0).all()) and bool((ref.prob[valid] <= 1.0).all())
    tie = U.CASES[U.CASE_IDS.index("tie")]
    inp, ref = U.ce_inputs("tie"), U.ce_ref("tie", False)
    assert torch.equal(inp.logits[:, U.TIE_LO], inp.logits[:, U.TIE_HI])
    assert not bool((ref.argmax == U.TIE_HI).any())
    n_tied = int((ref.argmax == U.TIE_LO).sum())
    assert n_tied >= ref.argmax.numel() // 4, "the tied pair must be the maximum at many pixels"
    # the tie rule decides the count: pixels labelled TIE_HI under a tied maximum are NOT correct
    assert int(((ref.argmax == U.TIE_LO) & (inp.labels == U.TIE_HI)).sum()) > 0
    assert int(((ref.argmax == U.TIE_LO) & (inp.labels == U.TIE_LO)).sum()) > 0
    assert tie.route[0] == "pow2"
    # an in-range ignore_index: raw labels equal to it still count towards #(argmax == label)
    case = U.CASES[U.CASE_IDS.index("ignore-in-range")]
    inp, ref = U.ce_inputs(case.name), U.ce_ref(case.name, False)
    assert int(((ref.argmax == case.ignore) & (inp.labels == case.ignore)).sum()) > 0
