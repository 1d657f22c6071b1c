"""gs_window_attention_*, gs_map_pad / gs_map_crop and gs_cell_layernorm_* through the C-ABI
(csrc/window_attention.hip), under the protocol of tests/test_attention_kv_gpu.py with the harness of
tests/util_attention_gpu.py: sentinel-filled outputs, NaN-filled pads and idle heads, a NaN-filled workspace of
exactly the queried size in front of a guard, two runs that must agree bit for bit, an accumulate run that equals
base + plain, and TOL = 3e-5 in conftest.rel_err against float64 (the project's bound for fp32 operators;
tests/test_swin.py checks on the CPU that float32 torch stays below 1e-5 on these inputs).

A one-wave workgroup handles one (window, head): ws^2 tokens padded to 64.  The backward cuts the (batch, window)
items into S slabs and sums the slabs' table partials in slab order in a second launch."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_swin as S
from util_attention_gpu import DEV, GS_E_BADARG, NAN, SENTINEL, Workspace, active, padded, stream

pytestmark = pytest.mark.gpu
TOL = 3e-5
HW = S.HEAD_DIM * 4   # a sliced operand's width: 4 heads
NAMES = ("O", "lse", "dQ", "dK", "dV", "dTable", "dQ+", "dK+", "dV+", "dTable+")


def _sliced(ts, fill):
    """three [b, n, c] tensors as column slices (HW apart) of one buffer filled with ``fill``"""
    b, n, c = ts[0].shape
    buf = torch.full((b, n, 3 * HW), fill)
    for i, t in enumerate(ts):
        buf[..., i * HW:i * HW + c] = t
    buf = buf.to(DEV)
    return buf, [buf.data_ptr() + 4 * i * HW for i in range(3)]


def _unslice(buf, c, what):
    full = buf.cpu()
    outside = torch.ones_like(full, dtype=torch.bool)
    for i in range(3):
        outside[..., i * HW:i * HW + c] = False
    assert bool((full[outside] == SENTINEL).all()), "%s: a store outside the active columns" % what
    return [full[..., i * HW:i * HW + c].contiguous() for i in range(3)]


def run_wa(L, lib, b, h, w, ws, shift, heads, sliced, q, k, v, table, do, bases):
    """forward, backward (overwrite), backward (accumulate onto the bases) -> the ten tensors of NAMES.
    ``sliced``: Q, K, V (and dQ, dK, dV) are three column slices of one buffer 4 heads wide per operand, the
    idle columns holding NaN (inputs) / the sentinel (outputs), O / dO have a pitch wider than needed and the
    table has ld_table = heads + 2 with NaN in the idle columns."""
    c, n, rows = S.HEAD_DIM * heads, h * w, S.table_rows(ws)
    if sliced:
        qkv, (qp, kp, vp) = _sliced([q, k, v], NAN)
        ldq, ldo, ldt = 3 * HW, c + 24, heads + 2
    else:
        qkv = [t.contiguous().to(DEV) for t in (q, k, v)]
        qp, kp, vp = (t.data_ptr() for t in qkv)
        ldq, ldo, ldt = c, c, heads
    tg = padded(table, ldt, NAN)
    d = lib.window_attention_desc(b, h, w, ws, shift, heads, ld_table=ldt, scale=S.SCALE, ldq=ldq, ldk=ldq, ldv=ldq,
                                  ldo=ldo)
    db, st = ctypes.byref(d), stream()
    o = torch.full((b, n, ldo), SENTINEL, device=DEV)
    lse = torch.full((b * heads * n + 8,), SENTINEL, device=DEV)
    lib.check(L.gs_window_attention_forward(db, qp, kp, vp, tg.data_ptr(), o.data_ptr(), lse.data_ptr(), st), "wa fwd")
    o_got = active(o, 0, c, "O")
    lse_cpu = lse.cpu()
    assert bool((lse_cpu[b * heads * n:] == SENTINEL).all()), "lse: a store past [B][heads][H*W]"
    lse_got = lse_cpu[:b * heads * n].view(b, heads, n)
    assert bool(torch.isfinite(lse_got).all()), "lse: NaN"
    dog = padded(do, ldo, NAN)
    outs = []
    for accumulate in (0, 1):
        if sliced:
            g, (dqp, dkp, dvp) = _sliced(list(bases[:3]) if accumulate else
                                         [torch.full_like(t, SENTINEL) for t in bases[:3]], SENTINEL)
        else:
            gb = [(t.contiguous().to(DEV) if accumulate else torch.full(t.shape, SENTINEL, device=DEV))
                  for t in bases[:3]]
            dqp, dkp, dvp = (t.data_ptr() for t in gb)
        dt = padded(bases[3] if accumulate else torch.full((rows, heads), SENTINEL), ldt, SENTINEL)
        wsp = Workspace(L.gs_window_attention_workspace_bytes(db))
        lib.check(L.gs_window_attention_backward(db, qp, kp, vp, tg.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                 dog.data_ptr(), dqp, dkp, dvp, dt.data_ptr(), accumulate, wsp.ptr(),
                                                 wsp.need, st), "wa bwd")
        wsp.check()
        got = _unslice(g, c, "dQ / dK / dV") if sliced else [t.cpu() for t in gb]
        got.append(active(dt, 0, heads, "dTable"))
        for name, t in zip(("dQ", "dK", "dV", "dTable"), got):
            assert bool(torch.isfinite(t).all()), "%s: NaN -- a pad column or unwritten scratch was read" % name
        outs += got
    del qkv
    return (o_got, lse_got) + tuple(outs)


def _want(q, k, v, table, do, geom, bases):
    ref = S.wa_ref(q, k, v, table, do, *geom)
    return ref + tuple(r + base.double() for r, base in zip(ref[2:], bases))


def _check(label, first, second, want):
    print(label, {nm: "%.2e" % rel_err(g, r) for nm, g, r in zip(NAMES, first, want)})
    for nm, a, bb in zip(NAMES, first, second):
        assert torch.equal(a, bb), "%s: %s differs between two runs" % (label, nm)
    for nm, g, r in zip(NAMES, first, want):
        assert rel_err(g, r) < TOL, "%s: %s: rel_err %.3g" % (label, nm, rel_err(g, r))


@pytest.mark.parametrize("case", S.WA_CASES, ids=[c[0] for c in S.WA_CASES])
def test_window_attention_forward_backward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, h, w, ws, shift, heads, sliced, dominant = case
    q, k, v, do, bases, table = S.wa_inputs(b, h, w, ws, heads, dominant, 5)
    want = _want(q, k, v, table, do, (b, h, w, ws, shift, heads), bases)
    first = run_wa(hip_lib, lib, b, h, w, ws, shift, heads, sliced, q, k, v, table, do, bases)
    second = run_wa(hip_lib, lib, b, h, w, ws, shift, heads, sliced, q, k, v, table, do, bases)
    _check(name, first, second, want)


def test_window_attention_table_split(hip_lib):
    """40 windows on S = 1, 2, 3, 40 slabs: every S within TOL, bit-identical between two runs, the workspace
    (which grows with S) not overrun"""
    from gaia_seg_amd.hip import lib
    L = hip_lib
    b, h, w, ws, shift, heads = S.SPLIT_CASE
    q, k, v, do, bases, table = S.wa_inputs(b, h, w, ws, heads, False, 9)
    want = _want(q, k, v, table, do, S.SPLIT_CASE, bases)
    d = lib.window_attention_desc(b, h, w, ws, shift, heads)
    sizes = []
    try:
        for s in S.SPLITS:
            assert L.gs_debug_set_window_attention_split(s) == 0
            sizes.append(L.gs_window_attention_workspace_bytes(ctypes.byref(d)))
            first = run_wa(L, lib, b, h, w, ws, shift, heads, False, q, k, v, table, do, bases)
            second = run_wa(L, lib, b, h, w, ws, shift, heads, False, q, k, v, table, do, bases)
            _check("S = %d (%d bytes)" % (s, sizes[-1]), first, second, want)
        assert L.gs_debug_set_window_attention_split(0) == GS_E_BADARG
        assert L.gs_debug_set_window_attention_split(-2) == GS_E_BADARG
    finally:
        assert L.gs_debug_set_window_attention_split(-1) == 0
    part = heads * S.table_rows(ws) * 4
    assert sizes == [-(-s * part // 16) * 16 for s in S.SPLITS], sizes


def test_window_attention_zero_table_no_shift(hip_lib):
    """a zero table and no shift: plain attention inside every window"""
    from gaia_seg_amd.hip import lib
    b, h, w, ws, shift, heads = 2, 14, 7, 7, 0, 2
    q, k, v, do, bases, table = S.wa_inputs(b, h, w, ws, heads, False, 3)
    table = torch.zeros_like(table)
    want = _want(q, k, v, table, do, (b, h, w, ws, shift, heads), bases)
    first = run_wa(hip_lib, lib, b, h, w, ws, shift, heads, False, q, k, v, table, do, bases)
    second = run_wa(hip_lib, lib, b, h, w, ws, shift, heads, False, q, k, v, table, do, bases)
    _check("zero table", first, second, want)


def test_map_pad_and_crop(hip_lib):
    """(2, 5, 6) -> (7, 7), C = 36 at pitch 40: the pad is exact and zero-filled, the crop of the pad is the
    input bit for bit, the accumulate form adds, nothing outside the active columns is written"""
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    b, h, w, hp, wp, c, ld = 2, 5, 6, 7, 7, 36, 40
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, h, w, c, generator=g)
    base = torch.randn(b, h, w, c, generator=g)
    xg = padded(x, ld, NAN)
    big = torch.full((b, hp, wp, ld), SENTINEL, device=DEV)
    lib.check(L.gs_map_pad(xg.data_ptr(), ld, big.data_ptr(), ld, b, h, w, hp, wp, c, 0, st), "pad")
    got = active(big, 0, c, "pad")
    want = torch.zeros(b, hp, wp, c)
    want[:, :h, :w] = x
    assert torch.equal(got, want)
    back = torch.full((b, h, w, ld), SENTINEL, device=DEV)
    lib.check(L.gs_map_crop(big.data_ptr(), ld, back.data_ptr(), ld, b, h, w, hp, wp, c, 0, st), "crop")
    assert torch.equal(active(back, 0, c, "crop"), x)
    acc = padded(base, ld, SENTINEL)
    lib.check(L.gs_map_crop(big.data_ptr(), ld, acc.data_ptr(), ld, b, h, w, hp, wp, c, 1, st), "crop +=")
    assert torch.equal(active(acc, 0, c, "crop +="), base + x)


@pytest.mark.parametrize("shape", [(2, 4, 6, 12, 20), (1, 2, 2, 4, 4)], ids=["2x4x6-c12-of-20", "1x2x2-c4"])
def test_cell_layernorm(hip_lib, shape):
    """the 2x2-cell LayerNorm against the float64 LayerNorm of transformers' concatenation: y, dx (plain and
    accumulated), dweight and dbias at g * Cmax + c, idle parameter columns untouched, two runs bit-identical"""
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    b, h, w, c, cmax = shape
    ld = c + 8
    g = torch.Generator().manual_seed(2)
    x, dy, base = (torch.randn(b, h, w, c, generator=g) for _ in range(3))
    weight, bias = 1 + 0.5 * torch.randn(4 * cmax, generator=g), torch.randn(4 * cmax, generator=g)
    xr = x.double().requires_grad_(True)
    wr, br = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    y_r = S.cell_ln_formula(xr, wr, br, c, cmax)
    y_r.backward(dy.double())
    # the formula is the LayerNorm of the concatenated phases
    cols = torch.cat([torch.arange(gq * cmax, gq * cmax + c) for gq in range(4)])
    ln = torch.nn.functional.layer_norm(S.merge_cat(x.double()), (4 * c,), weight.double()[cols], bias.double()[cols],
                                        1e-5)
    assert rel_err(S.merge_cat(y_r.detach()), ln) < 1e-12
    idle = torch.ones(4 * cmax, dtype=torch.bool)
    idle[cols] = False
    wn, bn = weight.clone(), bias.clone()
    wn[idle], bn[idle] = NAN, NAN
    d = lib.cell_layernorm_desc(b, h, w, c, cmax, 1e-5, ldx=ld, ldy=ld)
    db = ctypes.byref(d)
    runs = []
    for _ in range(2):
        xg, wg, bg = padded(x, ld, NAN), wn.to(DEV), bn.to(DEV)
        y = torch.full((b, h, w, ld), SENTINEL, device=DEV)
        stats = torch.full((2 * b * h * w // 4 + 8,), SENTINEL, device=DEV)
        cells = b * h * w // 4
        lib.check(L.gs_cell_layernorm_forward(db, xg.data_ptr(), wg.data_ptr(), bg.data_ptr(), y.data_ptr(),
                                              stats.data_ptr(), stats.data_ptr() + 4 * cells, st), "cell ln fwd")
        out = [active(y, 0, c, "y")]
        assert bool((stats.cpu()[2 * cells:] == SENTINEL).all())
        dyg = padded(dy, ld, NAN)
        for accumulate in (0, 1):
            dx = padded(base, ld, SENTINEL) if accumulate else torch.full((b, h, w, ld), SENTINEL, device=DEV)
            dw, dbs = (torch.full((4 * cmax,), SENTINEL, device=DEV) for _ in range(2))
            wsp = Workspace(L.gs_cell_layernorm_workspace_bytes(db))
            lib.check(L.gs_cell_layernorm_backward(db, xg.data_ptr(), dyg.data_ptr(), wg.data_ptr(), stats.data_ptr(),
                                                   stats.data_ptr() + 4 * cells, dx.data_ptr(), dw.data_ptr(),
                                                   dbs.data_ptr(), accumulate, wsp.ptr(), wsp.need, st), "cell ln bwd")
            wsp.check()
            out.append(active(dx, 0, c, "dx"))
            for nm, t in (("dweight", dw), ("dbias", dbs)):
                t = t.cpu()
                assert bool((t[idle] == SENTINEL).all()), "%s: an idle parameter column was written" % nm
                out.append(t[cols])
        runs.append(out)
    want = [y_r.detach(), xr.grad, wr.grad[cols], br.grad[cols], xr.grad + base.double(), wr.grad[cols], br.grad[cols]]
    names = ("y", "dx", "dweight", "dbias", "dx+", "dweight'", "dbias'")
    print({nm: "%.2e" % rel_err(a, r) for nm, a, r in zip(names, runs[0], want)})
    for nm, a, bb, r in zip(names, runs[0], runs[1], want):
        assert torch.equal(a, bb), "%s differs between two runs" % nm
        assert rel_err(a, r) < TOL, "%s: rel_err %.3g" % (nm, rel_err(a, r))


def test_map_pad_accumulates(hip_lib):
    """the accumulate form of the pad (the crop's backward onto an existing gradient): += on the leading part,
    the pad zone untouched"""
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    b, h, w, hp, wp, c = 1, 3, 2, 4, 4, 8
    g = torch.Generator().manual_seed(4)
    x, base = torch.randn(b, h, w, c, generator=g), torch.randn(b, hp, wp, c, generator=g)
    big = padded(base, c + 4, SENTINEL)
    lib.check(L.gs_map_pad(x.to(DEV).data_ptr(), c, big.data_ptr(), c + 4, b, h, w, hp, wp, c, 1, st), "pad +=")
    want = base.clone()
    want[:, :h, :w] += x
    assert torch.equal(active(big, 0, c, "pad +="), want)


def test_swin_ops_on_the_tape(hip_lib):
    """ops.map_pad -> ops.window_attention (q, k, v three column slices of one padded buffer) -> ops.map_crop, and
    ops.cell_layernorm, against the float64 restatement through autograd"""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    b, h, w, ws, shift, heads, hmax = 2, 5, 9, 7, 3, 2, 3
    hp, wp, c = 7, 14, S.HEAD_DIM * heads
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(b, h, w, 3 * c, generator=g)
    do = torch.randn(b, h, w, c, generator=g)
    table = (0.5 * torch.randn(S.table_rows(ws), hmax, generator=g))
    # float64: zero-pad, attend on the padded map, crop
    x64 = qkv.double().requires_grad_(True)
    t64 = table.double().requires_grad_(True)
    xp = torch.nn.functional.pad(x64, (0, 0, 0, wp - w, 0, hp - h)).reshape(b, hp * wp, 3 * c)
    o64, _ = S.wa_formula(xp[..., :c], xp[..., c:2 * c], xp[..., 2 * c:], t64, b, hp, wp, ws, shift, heads)
    o64 = o64.view(b, hp, wp, c)[:, :h, :w]
    o64.backward(do.double())
    tape = Tape()
    xa = Act(qkv.to(DEV))
    xa.requires_grad = True
    tp = torch.nn.Parameter(table.to(DEV))
    big = ops.map_pad(tape, xa, hp, wp)
    o = ops.window_attention(tape, big.slice(0, c), big.slice(c, 2 * c), big.slice(2 * c, 3 * c), tp, heads, ws, shift,
                             S.SCALE)
    out = ops.map_crop(tape, o, h, w)
    out.g = do.to(DEV)
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(out.t, o64.detach()) < TOL
    assert rel_err(xa.g, x64.grad) < TOL
    assert rel_err(tp.grad[:, :heads], t64.grad[:, :heads]) < TOL and not bool(tp.grad[:, heads:].any())
    # the cell LayerNorm
    cmax, cc = 12, 8
    x = torch.randn(b, 4, 6, cc, generator=g)
    dy = torch.randn(b, 4, 6, cc, generator=g)
    wt, bs = 1 + 0.5 * torch.randn(4 * cmax, generator=g), torch.randn(4 * cmax, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wt, bs))
    y_r = S.cell_ln_formula(xr, wr, br, cc, cmax)
    y_r.backward(dy.double())
    tape = Tape()
    xa = Act(x.to(DEV))
    xa.requires_grad = True
    wp_, bp_ = torch.nn.Parameter(wt.to(DEV)), torch.nn.Parameter(bs.to(DEV))
    y = ops.cell_layernorm(tape, xa, wp_, bp_)
    y.g = dy.to(DEV)
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(y.t, y_r.detach()) < TOL and rel_err(xa.g, xr.grad) < TOL
    assert rel_err(wp_.grad, wr.grad) < TOL and rel_err(bp_.grad, br.grad) < TOL
