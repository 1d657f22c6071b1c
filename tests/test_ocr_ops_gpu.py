"""OCRNet's two region operators through the C-ABI (gs_ocr_gather_*, gs_ocr_attend_*; csrc/ocr.hip) against
float64 (tests/util_ocr.py), under the protocol of tests/test_convnext_ops_gpu.py:

  * outputs are pre-filled with a sentinel: everything outside the written slice -- pad columns of a wide
    pitch, the other half of a concat buffer -- must still hold it;
  * pad columns of the inputs beyond the width hold NaN;
  * workspaces are exactly the queried size, hold NaN (0xFF), and sit in front of a 4 KiB guard;
  * every case runs twice and the two results are bit-identical (fixed reduction order, no atomics).

Bound: rel_err against float64 at TOL = 3e-5, the project's bound for fp32 operators (tests/test_dwconv_gpu.py),
with F, Q, Kr, V, dctx, dout ~ N(0, 1) and L ~ 3 N(0, 1).  Measured on the MI355X: at most 1.3e-6 over all cases.

Shapes (B, H x W, K, C or ch): 221 pixels are ragged runs of rows (64 for the statistics, 128 for the products)
with K = 19 at pitch 20; 667 pixels are eleven / six runs with a ragged tail and 18 quads, more than one
16-quad column group and a lane group narrower than a wave; K = 3 is below one float4; K = 150 at width 256
walks the classes in several LDS chunks with a whole wave per row.  Each shape runs once more with the
features as the upper half of a 2C-wide buffer and dF accumulated onto a pre-filled gradient (for the
attention: with every operand at a wider pitch of its own)."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_ocr as U
from test_convnext_ops_gpu import DEV, NAN, SENTINEL, TOL, Workspace, active, padded, stream

pytestmark = pytest.mark.gpu

# (B, H, W, K, C)
SHAPES = [(2, 13, 17, 19, 8), (2, 23, 29, 19, 72), (3, 23, 29, 3, 72), (2, 13, 17, 150, 256)]
CASES = [s + (sl,) for s in SHAPES for sl in (False, True)]


def case_id(c):
    return "%dx%dx%d-k%d-c%d%s" % (c[:5] + ("-slice-acc" if c[5] else "",))


def up4(n):
    return (n + 3) // 4 * 4


def run_gather(L, lib, logits, feats, scale, dctx, base, sliced):
    """forward and backward through the library handle L: ctx, stats, dfeats, dlogits (CPU, active columns).
    ``sliced``: feats and dfeats are columns [C, 2C) of a 2C-wide buffer, and dfeats accumulates onto base."""
    b, p, k = logits.shape
    c = feats.shape[2]
    ldl, lddl = up4(k), up4(k) + 4
    ldf, c0 = (2 * c, c) if sliced else (c + 4, 0)
    ldc, lddc = c + 4, c + 8
    d = lib.ocr_gather_desc(b, p, k, c, scale, ldl=ldl, ldf=ldf, ldc=ldc, lddl=lddl, lddf=ldf, lddc=lddc)
    db, st = ctypes.byref(d), stream()
    lg = padded(logits.reshape(b * p, k), ldl, NAN)
    fg = padded(feats.reshape(b * p, c), ldf, NAN, c0)
    dcg = padded(dctx.reshape(b * k, c), lddc, NAN)
    ctx = torch.full((b * k, ldc), SENTINEL, device=DEV)
    stats = torch.full((b * k * 2 + 16,), SENTINEL, device=DEV)
    need = L.gs_ocr_gather_workspace_bytes(db)
    ws = Workspace(need)
    lib.check(L.gs_ocr_gather_forward(db, lg.data_ptr(), fg.data_ptr() + 4 * c0, ctx.data_ptr(), stats.data_ptr(),
                                      ws.ptr(), ws.need, st), "gather fwd")
    got_ctx = active(ctx, 0, c, "ctx")
    got_stats = active(stats, 0, b * k * 2, "stats").view(b, k, 2)
    ws.check()
    ws = Workspace(need)
    dl = torch.full((b * p, lddl), SENTINEL, device=DEV)
    df = (padded(base.reshape(b * p, c), ldf, SENTINEL, c0) if sliced
          else torch.full((b * p, ldf), SENTINEL, device=DEV))
    lib.check(L.gs_ocr_gather_backward(db, lg.data_ptr(), fg.data_ptr() + 4 * c0, ctx.data_ptr(), stats.data_ptr(),
                                       dcg.data_ptr(), dl.data_ptr(), df.data_ptr() + 4 * c0, 1 if sliced else 0,
                                       ws.ptr(), ws.need, st), "gather bwd")
    got_df = active(df, c0, c, "dfeats")
    got_dl_padded = active(dl, 0, up4(k), "dlogits")
    assert bool((got_dl_padded[:, k:] == 0).all()), "dlogits: the pad columns of the float4 pitch are not zero"
    ws.check()
    return (got_ctx.view(b, k, c), got_stats, got_df.view(b, p, c), got_dl_padded[:, :k].reshape(b, p, k))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gather_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    b, h, w, k, c, sliced = case
    p = h * w
    gen = torch.Generator().manual_seed(71 + k + c)
    logits = 3.0 * torch.randn(b, p, k, generator=gen)
    feats, base = torch.randn(b, p, c, generator=gen), torch.randn(b, p, c, generator=gen)
    dctx = torch.randn(b, k, c, generator=gen)
    scale = 1.0 if not sliced else 0.5
    ctx_r, stats_r, df_r, dl_r = U.gather_ref(logits, feats, scale, dctx)
    want = (ctx_r, stats_r, df_r + base.double() if sliced else df_r, dl_r)
    first = run_gather(hip_lib, lib, logits, feats, scale, dctx, base, sliced)
    second = run_gather(hip_lib, lib, logits, feats, scale, dctx, base, sliced)
    for name, a, a2, r in zip(("ctx", "stats", "dfeats", "dlogits"), first, second, want):
        err = rel_err(a, r)
        print("gather %s: %s rel_err %.3g" % (case_id(case), name, err))
        assert err < TOL, name
        assert torch.equal(a, a2), "%s: two runs of the same input differ" % name


def test_gather_with_zero_scale_is_the_exact_pixel_mean(hip_lib):
    """s = 0 makes every softmax weight 1 / P; with P = 16 x 16 a power of two and small-integer features every
    partial sum is an integer below 2^24 and the division is exact: torch.equal against float64"""
    from gaia_seg_amd.hip import lib
    b, p, k, c = 2, 256, 19, 8
    gen = torch.Generator().manual_seed(5)
    logits = torch.randint(-3, 4, (b, p, k), generator=gen).float()
    feats = torch.randint(-3, 4, (b, p, c), generator=gen).float()
    dctx = torch.randint(-3, 4, (b, k, c), generator=gen).float()
    ctx = run_gather(hip_lib, lib, logits, feats, 0.0, dctx, torch.zeros(b, p, c), False)[0]
    want = feats.double().mean(dim=1, keepdim=True).expand(b, k, c)
    assert torch.equal(ctx.double(), want)
    assert torch.equal(ctx.double(), U.gather_ref(logits, feats, 0.0, dctx)[0])


def run_attend(L, lib, q, k, v, dout, pitched):
    """forward and backward: out, lse, dq, dk, dv (CPU, active columns)"""
    b, p, ch = q.shape
    kk = k.shape[1]
    pad = (4, 8, 12, 16, 20, 4, 8, 12) if pitched else (0,) * 8
    ldq, ldk, ldv, ldo, lddq, lddk, lddv, lddo = (ch + x for x in pad)
    d = lib.ocr_attend_desc(b, p, kk, ch, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddq=lddq, lddk=lddk, lddv=lddv,
                            lddo=lddo)
    db, st = ctypes.byref(d), stream()
    qg, kg, vg = (padded(t.reshape(-1, ch), ld, NAN) for t, ld in ((q, ldq), (k, ldk), (v, ldv)))
    dog = padded(dout.reshape(b * p, ch), lddo, NAN)
    out = torch.full((b * p, ldo), SENTINEL, device=DEV)
    lse = torch.full((b * p + 16,), SENTINEL, device=DEV)
    lib.check(L.gs_ocr_attend_forward(db, qg.data_ptr(), kg.data_ptr(), vg.data_ptr(), out.data_ptr(),
                                      lse.data_ptr(), st), "attend fwd")
    got_out, got_lse = active(out, 0, ch, "out"), active(lse, 0, b * p, "lse")
    dq = torch.full((b * p, lddq), SENTINEL, device=DEV)
    dk = torch.full((b * kk, lddk), SENTINEL, device=DEV)
    dv = torch.full((b * kk, lddv), SENTINEL, device=DEV)
    ws = Workspace(L.gs_ocr_attend_workspace_bytes(db))
    lib.check(L.gs_ocr_attend_backward(db, qg.data_ptr(), kg.data_ptr(), vg.data_ptr(), out.data_ptr(),
                                       lse.data_ptr(), dog.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                       ws.ptr(), ws.need, st), "attend bwd")
    res = (got_out.view(b, p, ch), got_lse.view(b, p), active(dq, 0, ch, "dq").view(b, p, ch),
           active(dk, 0, ch, "dk").view(b, kk, ch), active(dv, 0, ch, "dv").view(b, kk, ch))
    ws.check()
    return res


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_attend_kernels(hip_lib, case):
    """(the second run of a shape: every operand at a wider pitch of its own)"""
    from gaia_seg_amd.hip import lib
    b, h, w, kk, ch, pitched = case
    p = h * w
    gen = torch.Generator().manual_seed(91 + kk + ch)
    q, dout = torch.randn(b, p, ch, generator=gen), torch.randn(b, p, ch, generator=gen)
    k, v = torch.randn(b, kk, ch, generator=gen), torch.randn(b, kk, ch, generator=gen)
    want = U.attend_ref(q, k, v, dout)
    first = run_attend(hip_lib, lib, q, k, v, dout, pitched)
    second = run_attend(hip_lib, lib, q, k, v, dout, pitched)
    for name, a, a2, r in zip(("out", "lse", "dq", "dk", "dv"), first, second, want):
        err = rel_err(a, r)
        print("attend %s: %s rel_err %.3g" % (case_id(case), name, err))
        assert err < TOL, name
        assert torch.equal(a, a2), "%s: two runs of the same input differ" % name
