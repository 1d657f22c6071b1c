"""gs_attention_kv_* through the C-ABI (csrc/attention_common.h on two lengths), under the protocol of
tests/test_attention_gpu.py with the harness of tests/util_attention_gpu.py: sentinel-filled outputs,
NaN-filled pads and idle heads, a NaN-filled workspace of exactly the queried size in front of a guard, two
runs that must agree bit for bit, and TOL = 3e-5 in conftest.rel_err against float64 (that file's bound for
fp32 operators; tests/test_mit.py checks on the CPU that float32 torch stays below 1e-5 on these inputs).

A workgroup owns 128 rows (queries in the forward and dQ, keys in dK / dV) and sweeps the other operand in
tiles of 32; the dK / dV kernel splits the queries into S slabs of whole tiles and, for S > 1, sums the slabs'
partials in slab order in a second launch."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_mit as M
import util_vit as U
from util_attention_gpu import (DEV, GS_E_BADARG, NAMES, NAN, SENTINEL, Workspace, active, padded, run_attention,
                                stream)

pytestmark = pytest.mark.gpu
TOL = 3e-5
HW = 64 * 4   # a sliced operand's width: 4 heads, the 4th idle


def _sliced(ts, fill):
    """[b, n, c] tensors as column slices (HW apart) of one buffer filled with ``fill`` -> (buffer, pointers)"""
    b, n, c = ts[0].shape
    buf = torch.full((b, n, len(ts) * HW), fill)
    for i, t in enumerate(ts):
        buf[..., i * HW:i * HW + c] = t
    buf = buf.to(DEV)
    return buf, [buf.data_ptr() + 4 * i * HW for i in range(len(ts))]


def _unslice(buf, count, c, what):
    """the slices back on the CPU; everything between them still holds the sentinel"""
    full = buf.cpu()
    outside = torch.ones_like(full, dtype=torch.bool)
    for i in range(count):
        outside[..., i * HW:i * HW + c] = False
    assert bool((full[outside] == SENTINEL).all()), "%s: a store outside the active columns" % what
    return [full[..., i * HW:i * HW + c].contiguous() for i in range(count)]


def run_kv(L, lib, b, nq, nk, heads, sliced, q, k, v, do, bases):
    """forward, backward (overwrite), backward (accumulate onto the bases) of gs_attention_kv_* -> (O, lse, dQ,
    dK, dV, dQ+, dK+, dV+).  ``sliced``: Q (and dQ) is a column slice of a buffer 4 heads wide and K, V (and
    dK, dV) are two slices of one such buffer, the idle columns holding NaN (inputs) / the sentinel
    (outputs), and O / dO have a pitch wider than needed."""
    c = 64 * heads
    if sliced:
        qbuf, (qp,) = _sliced([q], NAN)
        kvbuf, (kp, vp) = _sliced([k, v], NAN)
        ldq, ldk, ldo = HW, 2 * HW, c + 24
    else:
        qbuf, kvbuf = q.contiguous().to(DEV), (k.contiguous().to(DEV), v.contiguous().to(DEV))
        qp, kp, vp = qbuf.data_ptr(), kvbuf[0].data_ptr(), kvbuf[1].data_ptr()
        ldq = ldk = ldo = c
    d = lib.attention_kv_desc(b, nq, nk, heads, U.SCALE, ldq=ldq, ldk=ldk, ldv=ldk, ldo=ldo)
    db, st = ctypes.byref(d), stream()
    o = torch.full((b, nq, ldo), SENTINEL, device=DEV)
    lse = torch.full((b * heads * nq + 8,), SENTINEL, device=DEV)
    lib.check(L.gs_attention_kv_forward(db, qp, kp, vp, o.data_ptr(), lse.data_ptr(), st), "kv fwd")
    o_got = active(o, 0, c, "O")
    lse_cpu = lse.cpu()
    assert bool((lse_cpu[b * heads * nq:] == SENTINEL).all()), "lse: a store past [B][heads][Nq]"
    lse_got = lse_cpu[:b * heads * nq].view(b, heads, nq)
    dog = padded(do, ldo, NAN)
    outs = []
    for accumulate in (0, 1):
        if sliced:
            fill = [torch.full_like(t, SENTINEL) for t in bases]
            gq, (dqp,) = _sliced([bases[0] if accumulate else fill[0]], SENTINEL)
            gkv, (dkp, dvp) = _sliced(list(bases[1:]) if accumulate else fill[1:], SENTINEL)
        else:
            gb = [(t.contiguous().to(DEV) if accumulate else torch.full(t.shape, SENTINEL, device=DEV)) for t in bases]
            dqp, dkp, dvp = (t.data_ptr() for t in gb)
        ws = Workspace(L.gs_attention_kv_workspace_bytes(db))
        lib.check(L.gs_attention_kv_backward(db, qp, kp, vp, o.data_ptr(), lse.data_ptr(), dog.data_ptr(), dqp, dkp,
                                             dvp, accumulate, ws.ptr(), ws.need, st), "kv bwd")
        ws.check()
        got = _unslice(gq, 1, c, "dQ") + _unslice(gkv, 2, c, "dK / dV") if sliced else [t.cpu() for t in gb]
        for name, t in zip(("dQ", "dK", "dV"), got):
            assert bool(torch.isfinite(t).all()), "%s: NaN -- a pad column or unwritten scratch was read" % name
        outs += got
    del qbuf, kvbuf
    return (o_got, lse_got) + tuple(outs)


def _want(q, k, v, do, heads, bases):
    o_r, lse_r, dq_r, dk_r, dv_r = M.kv_ref(q, k, v, do, heads)
    return (o_r, lse_r, dq_r, dk_r, dv_r, dq_r + bases[0].double(), dk_r + bases[1].double(),
            dv_r + bases[2].double())


@pytest.mark.parametrize("case", M.KV_CASES, ids=[c[0] for c in M.KV_CASES])
def test_attention_kv_forward_backward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, nq, nk, heads, sliced, dominant = case
    q, k, v, do, bq, bk, bv = M.kv_inputs(b, nq, nk, heads, dominant, 5)
    want = _want(q, k, v, do, heads, (bq, bk, bv))
    first = run_kv(hip_lib, lib, b, nq, nk, heads, sliced, q, k, v, do, (bq, bk, bv))
    second = run_kv(hip_lib, lib, b, nq, nk, heads, sliced, q, k, v, do, (bq, bk, bv))
    names = NAMES
    print(name, {nm: "%.2e" % rel_err(g, r) for nm, g, r in zip(names, first, want)})
    for nm, a, bb in zip(names, first, second):
        assert torch.equal(a, bb), "%s differs between two runs" % nm
    if nq == 1 and nk == 1:   # softmax of one element: O = V, and dP == delta bit for bit
        assert torch.equal(first[0], v), "single query and key: O != V"
        assert torch.equal(first[4], do), "single query and key: dV != dO"
        assert not bool(first[2].any()) and not bool(first[3].any()), "single: dQ, dK must be exactly 0"
        names, first, want = names[:2] + names[4:], first[:2] + first[4:], want[:2] + want[4:]
    for nm, g, r in zip(names, first, want):
        assert rel_err(g, r) < TOL, "%s: rel_err %.3g" % (nm, rel_err(g, r))


def test_attention_kv_query_split(hip_lib):
    """the dK / dV kernel on S = 1, 2, 3, 10 slabs of the queries (ten tiles: S = 10 is one tile per slab, the
    last one ragged): every S within TOL, bit-identical between two runs, the workspace (which grows with S)
    not overrun, accumulate == base + plain"""
    from gaia_seg_amd.hip import lib
    L = hip_lib
    b, nq, nk, heads = M.SPLIT_CASE
    q, k, v, do, bq, bk, bv = M.kv_inputs(b, nq, nk, heads, False, 9)
    want = _want(q, k, v, do, heads, (bq, bk, bv))
    d = lib.attention_kv_desc(b, nq, nk, heads, U.SCALE)
    sizes = []
    try:
        for s in M.SPLITS:
            assert L.gs_debug_set_attention_kv_split(s) == 0
            sizes.append(L.gs_attention_kv_workspace_bytes(ctypes.byref(d)))
            first = run_kv(L, lib, b, nq, nk, heads, False, q, k, v, do, (bq, bk, bv))
            second = run_kv(L, lib, b, nq, nk, heads, False, q, k, v, do, (bq, bk, bv))
            print("S = %d (%d bytes)" % (s, sizes[-1]), {nm: "%.2e" % rel_err(g, r)
                                                         for nm, g, r in zip(NAMES, first, want)})
            for nm, a, bb, r in zip(NAMES, first, second, want):
                assert torch.equal(a, bb), "S = %d: %s differs between two runs" % (s, nm)
                assert rel_err(a, r) < TOL, "S = %d: %s: rel_err %.3g" % (s, nm, rel_err(a, r))
            for plain, plus, base in zip(first[3:5], first[6:8], (bk, bv)):
                assert rel_err(plus, plain.double() + base.double()) < TOL
        assert L.gs_debug_set_attention_kv_split(0) == GS_E_BADARG and L.gs_debug_set_attention_kv_split(-2) == GS_E_BADARG
    finally:
        assert L.gs_debug_set_attention_kv_split(-1) == 0
    delta = 4 * b * heads * nq
    part = 2 * b * nk * 64 * heads * 4
    assert sizes == [delta] + [delta + s * part for s in M.SPLITS[1:]], sizes


def test_attention_kv_equals_self_attention_bits(hip_lib):
    """Nq == Nk, one slab, the same operands: all eight outputs equal gs_attention_* bit for bit"""
    from gaia_seg_amd.hip import lib
    L = hip_lib
    try:
        assert L.gs_debug_set_attention_kv_split(1) == 0
        for b, n, heads, sliced in ((2, 129, 3, False), (1, 265, 3, True)):
            q, k, v, do, bq, bk, bv = U.attention_inputs(b, n, heads, False, 5)
            got = run_kv(L, lib, b, n, n, heads, sliced, q, k, v, do, (bq, bk, bv))
            old = run_attention(L, lib, b, n, heads, sliced, q, k, v, do, (bq, bk, bv))
            for nm, a, bb in zip(NAMES, got, old):
                assert torch.equal(a, bb), "%s differs from gs_attention_* at N = %d" % (nm, n)
    finally:
        assert L.gs_debug_set_attention_kv_split(-1) == 0


def test_attention_kv_op_on_the_tape(hip_lib):
    """ops.attention_kv: q a map [B, Hq, Wq, C], k and v the two column slices of one reduced map's buffer
    (whose gradient is one zeroed buffer the kernels add to)"""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    b, hq, wq, hk, wk, heads = 2, 6, 8, 3, 2, 2
    c = 64 * heads
    q, k, v, do, bq, bk, bv = M.kv_inputs(b, hq * wq, hk * wk, heads, False, 13)
    _, _, dq_r, dk_r, dv_r = M.kv_ref(q, k, v, do, heads)
    o_r, _ = M.kv_formula(q.double(), k.double(), v.double(), heads)
    tape = Tape()
    qa = Act(q.view(b, hq, wq, c).contiguous().to(DEV))
    kv = Act(torch.cat([k, v], dim=-1).view(b, hk, wk, 2 * c).contiguous().to(DEV))
    ka, va = kv.slice(0, c), kv.slice(c, 2 * c)
    out = ops.attention_kv(tape, qa, ka, va, heads, U.SCALE)
    out.g = do.view(b, hq, wq, c).contiguous().to(DEV)
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(out.t.view(b, hq * wq, c), o_r) < TOL
    for name, a, r, n in (("dQ", qa, dq_r, hq * wq), ("dK", ka, dk_r, hk * wk), ("dV", va, dv_r, hk * wk)):
        assert rel_err(a.g.reshape(b, n, c), r) < TOL, name
