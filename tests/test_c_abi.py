"""The C-ABI shared library loads and exports every symbol declared in include/gaiaseg_hip.h, and
the ctypes binding agrees with the header (no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

from gaia_seg_amd.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gaiaseg_hip.h")


def _header_decls():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"typedef struct .*?\} \w+;", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(gs_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, args = m.group(2), m.group(3).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        decls[name] = n
    return decls


def test_header_and_binding_agree():
    decls = _header_decls()
    assert len(decls) >= 30
    assert set(decls) == set(lib.PROTOTYPES), (set(decls) ^ set(lib.PROTOTYPES))
    for name, nargs in decls.items():
        assert len(lib.PROTOTYPES[name][1]) == nargs, name


def test_library_exports_every_symbol():
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in _header_decls():
        assert hasattr(cdll, name), name


def test_load_binds_and_reports_identity():
    L = lib.load()
    assert L.gs_abi_version() == lib.ABI_VERSION
    assert L.gs_target_arch() == b"gfx950"
    assert lib.error_string(0) == "success"
    assert "NULL" in lib.error_string(-4)


def test_descriptor_struct_sizes_match_header():
    # gs_conv_desc: 14 int32 + 4 int64 + 4 int32 + 1 pointer ; gs_ce_desc: 6 int32 + 4 int64 + 2 int32
    assert ctypes.sizeof(lib.ConvDesc) == 14 * 4 + 4 * 8 + 4 * 4 + 8
    assert ctypes.sizeof(lib.CeDesc) == 6 * 4 + 4 * 8 + 2 * 4
    assert ctypes.sizeof(lib.SlideDesc) == 16 * 4


def test_conv_desc_is_the_one_constructor():
    """lib.conv_desc: defaults, the output size and the packed-NHWC strides; ops._conv_desc fills the
    same bytes for an activation of the same geometry."""
    import torch
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act
    d = lib.conv_desc(1, 5, 7, 8, 12, 3, stride=2, dil=2, ldx=12, ci_max=16, co_ld=16)
    assert (d.pad, d.Ho, d.Wo) == (2, 3, 4)
    assert (d.x_sn, d.x_sh, d.x_sw, d.x_sc) == (5 * 7 * 12, 7 * 12, 12, 1)
    assert (d.Ci_max, d.Co_ld, d.ldy) == (16, 16, 12)
    assert d.in_affine is None
    x = Act(torch.empty(1, 5, 7, 12)[..., :8])
    weight = torch.empty(3, 3, 16, 16).permute(3, 2, 0, 1)   # logical OIHW on HWIO storage
    assert bytes(ops._conv_desc(x, weight, 12, 2, 2, 2, 12)) == bytes(d)


def test_argument_validation_needs_no_gpu():
    """Bad descriptors are rejected before any launch (return codes, not exceptions)."""
    L = lib.load()
    d = lib.ConvDesc()
    assert L.gs_conv2d_workspace_bytes(ctypes.byref(d)) == 0
    assert L.gs_conv2d_forward(ctypes.byref(d), None, None, None, None, None, None, 0, None) == -1
    assert L.gs_sgd_step(None, None, None, 16, 0.1, 0.9, 0.0, 1.0, 0, None) == -4
    with pytest.raises(lib.HipLibraryError):
        lib.check(-3, "probe")


def test_product_path_fails_loudly_without_gpu_tensor():
    """There is no CPU fallback: CPU tensors are refused by every module forward."""
    import torch
    from gaia_seg_amd.core.bricks import DynamicBatchNorm2d, DynamicConv2d
    with pytest.raises(lib.HipLibraryError):
        DynamicConv2d(8, 8, 3, padding=1)(torch.randn(1, 8, 4, 4))
    with pytest.raises(lib.HipLibraryError):
        DynamicBatchNorm2d(8)(torch.randn(2, 8, 4, 4))


def _plan(L, M, N, K, max_splits=64):
    bm, bn, sp, ks = (ctypes.c_int32() for _ in range(4))
    assert L.gs_debug_query_plan(M, N, K, max_splits, ctypes.byref(bm), ctypes.byref(bn),
                                 ctypes.byref(sp), ctypes.byref(ks)) == 0
    return bm.value, bn.value, sp.value, ks.value


def test_conv_planner_invariants_need_no_gpu():
    """The tile / split-K cost model (csrc/igemm_core.h make_plan) is host arithmetic: check its
    invariants and a few decisions the r01 sweeps pinned down."""
    L = lib.load()
    shapes = [(65536, 64, 576), (16384, 128, 1152), (4096, 256, 2304), (1024, 512, 4608),
              (1024, 512, 18432), (4096, 192, 1728), (65536, 256, 64), (1024, 2048, 512), (99, 48, 1152)]
    for M, N, K in shapes:
        for ms in (64, 512):
            bm, bn, sp, ks = _plan(L, M, N, K, ms)
            nk = -(-K // 16)
            assert bm == 64 and bn in (80, 64, 48, 32)
            assert 1 <= sp <= ms and sp * ks >= nk and (sp - 1) * ks < nk     # K range covered exactly
            assert sp == 1 or ks >= 4                                          # no degenerate splits
            assert sp * M * N * 4 <= 96 << 20 or sp == 1                        # slab bound
            assert _plan(L, M, N, K, ms) == (bm, bn, sp, ks)                    # deterministic (cached)
    # a grid that already fills the chip several times over is never split
    assert _plan(L, 65536, 64, 576)[2] == 1
    assert _plan(L, 65536, 256, 64)[2] == 1
    # few tiles and a long K range: split until the workgroups make whole rounds of the 256 CUs
    bm, bn, sp, ks = _plan(L, 1024, 512, 18432)
    tiles = (1024 // 64) * -(-512 // bn)
    assert sp > 1 and (tiles * sp) % 256 == 0
    # the least-padded width wins when the tile count is comparable
    assert _plan(L, 16384, 96, 864)[1] == 48


def test_x3_dgrad_cases_pass_the_dispatch_gate_without_gpu():
    """The operator cases of tests/test_dgrad_x3_gpu.py are sized to reach the bf16x3 data-gradient
    loop.  gs_debug_query_conv_launch is host arithmetic, so the claim is checked here already (the
    GPU test re-checks it against the launch that really happened)."""
    if os.environ.get("GS_X3", "4") == "0":
        pytest.skip("bf16x3 switched off")
    from test_dgrad_x3_gpu import X3_CASES
    L = lib.load()
    seen_bn, seen_split, seen_odd = set(), False, False
    for case in X3_CASES:
        n, h, w, ci, co, k, dil, ci_max, co_ld, ldx, ldy, acc, force = case
        d = lib.conv_desc(n, h, w, ci, co, k, dil=dil, ci_max=ci_max, co_ld=co_ld, ldx=ldx, ldy=ldy)
        if force:
            assert L.gs_debug_force_plan(*force) == 0
        q = lib.DebugLaunch()
        try:
            assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_DGRAD, ctypes.byref(q)) == 0
        finally:
            L.gs_debug_force_plan(0, 0, 0)
        if case is X3_CASES[-1]:
            assert q.kloop != lib.KLOOP_BF16X3 and q.splits == 4 and q.ksteps_per_split < 48
            continue
        assert q.kloop == lib.KLOOP_BF16X3, case
        tiles = -(-n * h * w // 64) * -(-ci // q.bn) * q.splits
        assert q.bm == 64 and q.bn in (64, 48) and tiles >= 512 and q.ksteps_per_split >= 4
        seen_bn.add(q.bn)
        seen_split |= q.splits > 1 and q.ksteps_per_split >= 48
        seen_odd |= q.splits == 1 and q.ksteps_per_split % 2 == 1
    assert seen_bn == {64, 48} and seen_split and seen_odd
    # forward and weight gradient of a bf16x3 data-gradient shape stay on the fp32 loops
    d = lib.conv_desc(2, 64, 64, 1024, 256, 1)
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_DGRAD, ctypes.byref(q)) == 0
    assert q.kloop == lib.KLOOP_BF16X3
    for op in (lib.OP_FORWARD, lib.OP_WGRAD):
        assert L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q)) == 0
        assert q.kloop in (lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS) and q.op == op
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), 7, ctypes.byref(q)) == -1
    assert ctypes.sizeof(lib.DebugLaunch) == 8 * 4


def test_stream_1x1_cases_dispatch_without_gpu():
    """tests/test_stream_1x1_gpu.py's shapes reach the streaming 1x1 kernel (host arithmetic), the
    stage-3/4 shapes and the 3x3s do not."""
    if os.environ.get("GS_STREAM", "1") == "0":
        pytest.skip("streaming kernel switched off")
    from test_stream_1x1_gpu import STREAM_CASES
    L = lib.load()
    q = lib.DebugLaunch()
    widths = set()
    # production dispatch (mode 1): one column block, short data-gradient contractions
    d = _stream_desc(STREAM_CASES[0])     # 64 -> 256 at 2 x 128 x 256
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_FORWARD, ctypes.byref(q)) == 0
    assert q.kloop == lib.KLOOP_STREAM and q.bn == 256
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_DGRAD, ctypes.byref(q)) == 0
    assert q.kloop == lib.KLOOP_BF16X3    # K = 256: stays on the tile kernel's bf16x3 loop
    assert L.gs_debug_set_stream_mode(2) == 0 and L.gs_debug_set_stream_mode(5) == -1
    try:
        _stream_all_shapes(L, STREAM_CASES, q, widths)
    finally:
        L.gs_debug_set_stream_mode(-1)


def _stream_desc(case):
    n, h, w, ci, co, ci_max, co_ld, ldx, ldy = case[:9]
    return lib.conv_desc(n, h, w, ci, co, 1, ci_max=ci_max, co_ld=co_ld, ldx=ldx, ldy=ldy)


def _stream_all_shapes(L, STREAM_CASES, q, widths):
    for case in STREAM_CASES:
        d = _stream_desc(case)
        for op in case[-1]:
            assert L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q)) == 0
            assert q.kloop == lib.KLOOP_STREAM and q.bm == 128 and q.splits == 1, (case, op)
            widths.add(q.bn)
    assert widths == {64, 128, 256}
    for n, h, w, ci, co, k in [(2, 32, 64, 256, 1024, 1), (2, 16, 32, 2048, 512, 1), (2, 128, 256, 64, 64, 3),
                               (2, 64, 128, 512, 128, 1)]:
        d = lib.conv_desc(n, h, w, ci, co, k)
        assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_FORWARD, ctypes.byref(q)) == 0
        assert q.kloop != lib.KLOOP_STREAM


def test_wgrad_cases_make_their_coverage_claims_without_gpu():
    """tests/test_wgrad_gpu.py states per case which weight-gradient kernel, tile, split count (hence
    form of the reduce launch) and loader it is there for.  gs_debug_query_conv_launch is host
    arithmetic, so every claim is checked here already, and so is what the table covers as a whole (the
    GPU test re-checks each claim against the launch that really happened)."""
    import test_wgrad_gpu as T
    L = lib.load()
    seen_kloop, seen_bn = set(), {64: set(), 128: set()}
    seen_reduce, seen_walign, seen_aff = set(), set(), set()
    for c in T.ALL_CASES:
        d = T.make_desc(lib, c)
        if c.aff:
            d.in_affine = 4096          # any aligned address: the query does not read it
            assert L.gs_conv2d_in_affine_supported(ctypes.byref(d)) == (0 if T.NO_FAST else 1), c
        q = lib.DebugLaunch()
        with T.forced_plan(L, c):
            assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_WGRAD, ctypes.byref(q)) == 0
            need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        T.check_claim(c, d, q)
        m = d.KH * d.KW * c.ci
        assert need >= (q.splits * m * c.co * 4 if q.splits > 1 else 0)
        # the exact leg's integers stay exact in fp32: |x|, |dy| <= 3 (in_affine: activation <= 11)
        assert c.n * d.Ho * d.Wo * 3 * (11 if c.aff else 3) < 2 ** 22
        seen_kloop.add(q.kloop)
        seen_bn[q.bm].add(q.bn)
        seen_reduce.add((T.reduce_form(q.splits, m, c.co), q.splits >= 48))
        if c.walign and q.kloop != lib.KLOOP_GENERIC:
            seen_walign.add((c.stride, q.bm, q.kloop))
        if c.aff:
            seen_aff.add((q.kloop, c.walign))
    if T.NO_FAST:
        assert seen_kloop == {lib.KLOOP_GENERIC}
        return
    assert seen_bn[128] == {128, 96, 80, 64, 48, 32}
    assert seen_bn[64] >= {80, 64, 48, 32}
    assert {s for s, _, _ in seen_walign} >= {1, 2} and {b for _, b, _ in seen_walign} == {64, 128}
    if T.PLAN_ENV:
        return
    assert seen_kloop == {lib.KLOOP_GENERIC, lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS}
    # the reduce launch: none; sequential; WIDE for >= 48 splits; WIDE for 16..47 splits of few outputs
    assert seen_reduce >= {("none", False), ("seq", False), ("wide", True), ("wide", False)}
    assert {k for _, _, k in seen_walign} == {lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS}
    assert seen_aff >= {(lib.KLOOP_FP32, True), (lib.KLOOP_FP32, False), (lib.KLOOP_FP32_PAIRS, True)}


def test_conv_rows_cases_make_their_coverage_claims_without_gpu():
    """tests/test_conv_rows_gpu.py states per case and op which row kernel, K loop, tile, split count and
    form of the split-K reduce it is there for.  Every claim is checked here against
    gs_debug_query_conv_launch (host arithmetic; the GPU test re-checks it against the launch that really
    happened), and so is what the table covers as a whole, per op."""
    import test_conv_rows_gpu as T
    L = lib.load()
    FAST = (lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS)
    seen = {op: dict(kloop=set(), tiles=set(), reduce=set(), strides=set(), tapless=0, divs=set(), scalar=0,
                     aff=set()) for op in (T.FWD, T.DGRAD)}
    for c, op in T.PARAMS:
        d = T.make_desc(lib, c)
        if c.aff:
            d.in_affine = 4096          # any aligned address: the query does not read it
            assert L.gs_conv2d_in_affine_supported(ctypes.byref(d)) == (0 if T.NO_FAST else 1), c
        q = lib.DebugLaunch()
        with T.forced_plan(L, c):
            assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_FORWARD if op == T.FWD else lib.OP_DGRAD,
                                                ctypes.byref(q)) == 0
            need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        T.check_claim(L, lib, c, d, op, q)
        m, n, _ = T.gemm_dims(c, d, op)
        classes = T.in_classes(c, d, op)
        if classes:      # the largest slab among the classes' own plans
            recs = [T.class_record(L, lib, c, rows, taps) for _, _, rows, taps in T.dgrad_classes(c, d) if rows and taps]
            assert need >= max(r.splits * rows * n * 4 if r.splits > 1 else 0
                               for r, (_, _, rows, taps) in zip(recs, [x for x in T.dgrad_classes(c, d) if x[2] and x[3]]))
        else:
            assert need >= (q.splits * m * n * 4 if q.splits > 1 else 0), (c, op)
        assert T.exact_bound(c, d, op) < 2 ** 22
        s = seen[op]
        s["kloop"].add(q.kloop)
        if q.kloop in FAST:
            s["tiles"].add((q.bm, q.bn))
            if c.aff and op == T.FWD:
                s["aff"].add(q.kloop)
        if q.splits > 1 and not classes:
            # (form, an epilogue operand behind it, on the fast kernels); every data-gradient case runs = and +=
            for epi in ((c.bias or c.addend,) if op == T.FWD else (False, True)):
                s["reduce"].add(("launch" if T.combines(q) else "reduce", bool(epi), q.kloop in FAST))
        if op == T.DGRAD:
            if classes:
                s["strides"].add(c.stride)
                s["tapless"] += any(rows and not taps for _, _, rows, taps in T.dgrad_classes(c, d))
            elif q.kloop in FAST:
                s["strides"].add(1)
            elif c.stride > 1:
                s["divs"].add(3 if (d.KH, d.KW) == (3, 3) else (1 if (d.KH, d.KW) == (1, 1) else 0))
        elif not T.is_vector(c):
            s["scalar"] += 1
    if T.NO_FAST:
        assert all(s["kloop"] == {lib.KLOOP_GENERIC} for s in seen.values())
        return
    six = {128, 96, 80, 64, 48, 32}
    for op, s in seen.items():
        assert s["tiles"] >= {(bm, bn) for bm in (64, 128) for bn in six}, (op, s["tiles"])
    assert seen[T.FWD]["scalar"] >= 3
    assert seen[T.DGRAD]["strides"] >= {1, 2, 3} and seen[T.DGRAD]["tapless"] >= 1
    assert seen[T.DGRAD]["divs"] >= {3, 0}
    if T.PLAN_ENV or T.NO_COMBINE:
        return
    for op, s in seen.items():
        assert s["kloop"] == {lib.KLOOP_GENERIC, lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS}, op
        # both reduce forms behind the fast kernels, each with and without an epilogue operand, and the
        # reduce launch behind the generic kernel
        assert s["reduce"] >= {("launch", False, True), ("launch", True, True), ("reduce", False, True),
                               ("reduce", True, True), ("reduce", False, False)}, (op, s["reduce"])
    assert seen[T.FWD]["aff"] == {lib.KLOOP_FP32, lib.KLOOP_FP32_PAIRS}


def test_forward_and_dgrad_argument_checks_need_no_gpu():
    """gs_conv2d_forward and gs_conv2d_dgrad refuse bad arguments before any launch (every refusal of
    include/gaiaseg_hip.h, conv2d_forward_impl and conv2d_dgrad_impl).  The addresses are never read."""
    L = lib.load()
    OK_PTR, ODD_PTR = 1 << 20, (1 << 20) + 4
    E_BADARG, E_ALIGN, E_WORKSPACE, E_NULL = -1, -2, -3, -4

    def fwd(d, x=OK_PTR, w=OK_PTR, bias=None, addend=None, y=OK_PTR, ws=OK_PTR, ws_bytes=None):
        need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        return L.gs_conv2d_forward(ctypes.byref(d), x, w, bias, addend, y, ws, need if ws_bytes is None else ws_bytes,
                                   None)

    def dgrad(d, dy=OK_PTR, w=OK_PTR, dx=OK_PTR, acc=0, ws=OK_PTR, ws_bytes=None):
        need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        return L.gs_conv2d_dgrad(ctypes.byref(d), dy, w, dx, acc, ws, need if ws_bytes is None else ws_bytes, None)

    def shape(**kw):
        return lib.conv_desc(2, 13, 17, 48, 48, 3, **kw)     # 6 splits either way: needs slabs

    d, q = shape(), lib.DebugLaunch()
    slab = {}
    for op in (lib.OP_FORWARD, lib.OP_DGRAD):
        assert L.gs_debug_query_conv_launch(ctypes.byref(d), op, ctypes.byref(q)) == 0
        assert q.splits > 1
        slab[op] = q.splits * 2 * 13 * 17 * 48 * 4            # what the op itself needs
        assert 0 < slab[op] <= L.gs_conv2d_workspace_bytes(ctypes.byref(d))
    # ---- forward ----
    assert L.gs_conv2d_forward(None, OK_PTR, OK_PTR, None, None, OK_PTR, OK_PTR, slab[lib.OP_FORWARD], None) == E_NULL
    assert fwd(d, x=None) == E_NULL and fwd(d, w=None) == E_NULL and fwd(d, y=None) == E_NULL
    assert fwd(d, w=ODD_PTR) == E_ALIGN and fwd(d, y=ODD_PTR) == E_ALIGN
    assert fwd(d, bias=ODD_PTR) == E_ALIGN and fwd(shape(ld_add=48), addend=ODD_PTR) == E_ALIGN
    assert fwd(d, x=ODD_PTR) == E_ALIGN                      # a vector source is read as float4
    assert fwd(shape(ld_add=50), addend=OK_PTR) == E_ALIGN   # ld_add % 4
    assert fwd(shape(ld_add=44), addend=OK_PTR) == E_ALIGN   # ld_add < Co
    assert fwd(d, addend=OK_PTR) == E_ALIGN                  # ld_add = 0 beside an addend
    assert fwd(d, ws_bytes=slab[lib.OP_FORWARD] - 1) == E_WORKSPACE and fwd(d, ws=None) == E_WORKSPACE
    assert fwd(d, ws=None, ws_bytes=0) == E_WORKSPACE
    bad = shape()
    bad.Ho += 1
    assert fwd(bad) == E_BADARG
    # the descriptor's own alignment rules (check_desc)
    assert fwd(lib.conv_desc(2, 13, 17, 48, 46, 3)) == E_ALIGN                 # Co % 4
    assert fwd(shape(ldy=44)) == E_ALIGN                                        # ldy < Co
    assert fwd(shape(ci_max=32)) == E_BADARG                                    # Ci > Ci_max
    # in_affine: at most kAffMaxC = 640 channels, a vector source, a 1x1 or 3x3 ...
    for dims in [(2, 9, 9, 656, 64, 1), (2, 17, 19, 6, 24, 3), (1, 20, 24, 16, 32, 5)]:
        a = lib.conv_desc(*dims)
        a.in_affine = OK_PTR
        assert L.gs_conv2d_in_affine_supported(ctypes.byref(a)) == 0
        assert fwd(a) == E_BADARG, dims
    # ... and 64-row tiles: not under a forced 128-row plan
    a = lib.conv_desc(2, 9, 9, 640, 64, 1)
    a.in_affine = OK_PTR
    if L.gs_conv2d_in_affine_supported(ctypes.byref(a)) == 1:      # (not under GS_NO_FAST)
        assert L.gs_debug_force_plan(128, 64, 1) == 0
        try:
            assert L.gs_conv2d_in_affine_supported(ctypes.byref(a)) == 0
            assert fwd(a) == E_BADARG
        finally:
            L.gs_debug_force_plan(0, 0, 0)
        a.in_affine = ODD_PTR
        assert fwd(a) == E_ALIGN
    # ---- data gradient ----
    assert L.gs_conv2d_dgrad(None, OK_PTR, OK_PTR, OK_PTR, 0, OK_PTR, slab[lib.OP_DGRAD], None) == E_NULL
    assert dgrad(d, dy=None) == E_NULL and dgrad(d, w=None) == E_NULL and dgrad(d, dx=None) == E_NULL
    assert dgrad(d, dy=ODD_PTR) == E_ALIGN and dgrad(d, w=ODD_PTR) == E_ALIGN and dgrad(d, dx=ODD_PTR) == E_ALIGN
    assert dgrad(d, ws_bytes=slab[lib.OP_DGRAD] - 1) == E_WORKSPACE and dgrad(d, ws=None) == E_WORKSPACE
    assert dgrad(d, ws=None, ws_bytes=0) == E_WORKSPACE
    assert dgrad(bad) == E_BADARG
    nchw = shape()
    nchw.x_sn, nchw.x_sc, nchw.x_sh, nchw.x_sw = 48 * 13 * 17, 13 * 17, 17, 1
    assert dgrad(nchw) == E_ALIGN                                               # x_sc != 1
    assert dgrad(lib.conv_desc(2, 13, 17, 6, 48, 3)) == E_ALIGN                 # Ci % 4
    assert dgrad(shape(ldx=50)) == E_ALIGN                                      # x_sw % 4
    for field in ("x_sh", "x_sn"):                                              # dx is packed [N][H][W][x_sw]
        loose = shape(ldx=64)
        setattr(loose, field, getattr(loose, field) + 64)
        assert dgrad(loose) == E_BADARG, field
    # a strided data gradient in parity classes needs the largest class's slabs (+=: the call would
    # queue nothing in front of that check in any case)
    s2 = lib.conv_desc(2, 15, 15, 64, 256, 1, stride=2, pad=0)
    assert L.gs_debug_query_conv_launch(ctypes.byref(s2), lib.OP_DGRAD, ctypes.byref(q)) == 0
    if q.kloop != lib.KLOOP_GENERIC and q.splits > 1:
        assert dgrad(s2, acc=1, ws_bytes=q.splits * 2 * 8 * 8 * 64 * 4 - 1) == E_WORKSPACE
        assert dgrad(s2, acc=1, ws=None) == E_WORKSPACE


def test_wgrad_argument_checks_need_no_gpu():
    """gs_conv2d_wgrad refuses bad arguments before any launch.  (The addresses are never read.)"""
    L = lib.load()
    OK_PTR, ODD_PTR = 1 << 20, (1 << 20) + 4

    def call(d, x=OK_PTR, dy=OK_PTR, dw=OK_PTR, ws=OK_PTR, ws_bytes=None):
        need = L.gs_conv2d_workspace_bytes(ctypes.byref(d))
        return L.gs_conv2d_wgrad(ctypes.byref(d), x, dy, dw, ws, need if ws_bytes is None else ws_bytes, None)

    d = lib.conv_desc(2, 13, 17, 48, 48, 3)          # 7 splits: needs a slab
    q = lib.DebugLaunch()
    assert L.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_WGRAD, ctypes.byref(q)) == 0
    assert q.splits > 1
    slab = q.splits * 9 * 48 * 48 * 4                 # what the weight gradient itself needs
    assert 0 < slab <= L.gs_conv2d_workspace_bytes(ctypes.byref(d))
    assert L.gs_conv2d_wgrad(None, OK_PTR, OK_PTR, OK_PTR, OK_PTR, slab, None) == -4
    assert call(d, x=None) == -4 and call(d, dy=None) == -4 and call(d, dw=None) == -4      # GS_E_NULL
    assert call(d, dy=ODD_PTR) == -2 and call(d, dw=ODD_PTR) == -2                            # GS_E_ALIGN
    assert call(d, x=ODD_PTR) == -2                   # a vector source is read as float4
    assert call(d, ws_bytes=slab - 1) == -3 and call(d, ws=None) == -3                         # GS_E_WORKSPACE
    assert call(d, ws=None, ws_bytes=0) == -3
    bad = lib.conv_desc(2, 13, 17, 48, 48, 3)
    bad.Ho += 1
    assert call(bad) == -1
    # in_affine: at most kAffMaxC = 640 channels, a vector source, a 1x1 or 3x3
    for shape in [(2, 9, 9, 656, 64, 1), (2, 17, 19, 6, 24, 3), (1, 20, 24, 16, 32, 5)]:
        d = lib.conv_desc(*shape)
        d.in_affine = OK_PTR
        assert L.gs_conv2d_in_affine_supported(ctypes.byref(d)) == 0
        assert call(d) == -1, shape                                                            # GS_E_BADARG
    d = lib.conv_desc(2, 9, 9, 640, 64, 1)
    d.in_affine = ODD_PTR
    if L.gs_conv2d_in_affine_supported(ctypes.byref(d)) == 1:      # (not under GS_NO_FAST)
        assert call(d) == -2
