"""gs_attention_*_f16 through the C-ABI (csrc/attention_f16.hip) under the guards of
tests/test_attention_gpu.py -- sentinels outside the active columns, NaN in pad columns and in the idle head,
a workspace of exactly the queried size in front of a guard, two runs bit-identical -- and the tolerance
protocol of DESIGN.md section 32: the reference is float64 on the same fp32 inputs
(util_vit.attention_ref, conftest.rel_err) and every quantity must be within util_attention_f16.FACTOR (3)
times the error of the CPU witness (float64 with the kernels' rounding points) for that quantity, computed
at run time on the same inputs.

Observed / witness ratios on one MI355X (profiles/r19_fp16_attention.md): 0.92 .. 1.00."""
import ctypes
import math

import pytest
import torch

from conftest import rel_err
import util_attention_f16 as W
import util_beit as B
import util_vit as U
from util_attention_gpu import (DEV, GS_E_ALIGN, GS_E_BADARG, GS_E_NULL, GS_E_WORKSPACE, NAMES, RELPOS_CASES,
                                SENTINEL, make_table, stream)
import util_attention_gpu as A

pytestmark = pytest.mark.gpu
SEED = 1


def run_attention(L, lib, b, n, heads, sliced, q, k, v, do, bases, sfx="_f16", scale=U.SCALE):
    return A.run_attention(L, lib, b, n, heads, sliced, q, k, v, do, bases, sfx=sfx, scale=scale)


def check_budget(name, names, got, wit, want, norm=None):
    """every quantity within FACTOR x the witness's error; prints observed, witness and their ratio.
    ``norm``: compare in absolute terms divided by it (for quantities that are 0 in exact arithmetic)"""
    bad = []
    for nm, g, w, r in zip(names, got, wit, want):
        if norm is None:
            e_got, e_wit = rel_err(g, r), rel_err(w, r)
        else:
            e_got, e_wit = (float((t.double() - r.double()).abs().max()) / norm for t in (g, w))
        print("%s %s: observed %.3e witness %.3e ratio %.2f" % (name, nm, e_got, e_wit, e_got / max(e_wit, 1e-300)))
        if not e_got <= W.FACTOR * e_wit:
            bad.append("%s: %.3e > %g x %.3e" % (nm, e_got, W.FACTOR, e_wit))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


@pytest.mark.parametrize("case", U.ATTENTION_CASES, ids=[c[0] for c in U.ATTENTION_CASES])
def test_attention_f16_forward_backward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, n, heads, sliced, dominant = case
    q, k, v, do, bq, bk, bv = U.attention_inputs(b, n, heads, dominant, SEED)
    bases = (bq, bk, bv)
    ref = U.attention_ref(q, k, v, do, heads)
    wit = W.witness(q, k, v, do, heads)
    want = ref + tuple(r + t.double() for r, t in zip(ref[2:], bases))
    wit = wit + tuple(w + t.double() for w, t in zip(wit[2:], bases))
    first = run_attention(hip_lib, lib, b, n, heads, sliced, q, k, v, do, bases)
    second = run_attention(hip_lib, lib, b, n, heads, sliced, q, k, v, do, bases)
    for nm, t, u in zip(NAMES, first, second):
        assert bool(torch.isfinite(t).all()), "%s: not finite" % nm
        assert torch.equal(t, u), "%s differs between two runs" % nm
    if n == 1:   # dQ and dK are 0 in exact arithmetic: absolute, in units of max|dV|
        zero = [i for i, nm in enumerate(NAMES) if nm[:2] in ("dQ", "dK")]
        pick = lambda seq, idx: [seq[i] for i in idx]   # noqa: E731
        check_budget(name, pick(NAMES, zero), pick(first, zero), pick(wit, zero), pick(want, zero),
                     norm=float(ref[4].abs().max()))
        rest = [i for i in range(len(NAMES)) if i not in zero]
        check_budget(name, pick(NAMES, rest), pick(first, rest), pick(wit, rest), pick(want, rest))
    else:
        check_budget(name, NAMES, first, wit, want)
        assert rel_err(first[0], ref[0]) > 1e-4, "O is fp32-accurate: the fp16 kernel did not run"


def test_operand_layout_with_integer_data(hip_lib):
    """Exact check of the permuted k order of the P V product and of the transposed V image: N = 48 (the
    second key tile is ragged, its k-steps half filled), keys in three classes of 16 marked by a one-hot
    component of -64, queries with 8 on the components of the classes they exclude, scale 1/8: an excluded
    score is -64 and an allowed one 0, so P is 1 on 32 or 16 keys and exp(-64) (0 in fp16, and below half an
    ulp of the fp32 row sum) elsewhere.  V holds positive integers up to 8 that depend on the key and the
    column asymmetrically; every sum is an integer below 2^11 and the counts are powers of two, so O is the
    exact mean bit for bit and lse = log(count)."""
    from gaia_seg_amd.hip import lib
    n, c = 48, 64
    cls_k = torch.arange(n) // 16
    k = torch.zeros(1, n, c)
    k[0, torch.arange(n), cls_k] = -64.0
    q = torch.zeros(1, n, c)
    allowed = torch.zeros(n, n, dtype=torch.bool)
    for i in range(n):
        excl = [(i // 3) % 3] if i % 3 == 0 else [j for j in range(3) if j != (i + i // 3) % 3]
        q[0, i, excl] = 8.0
        allowed[i] = ~torch.isin(cls_k, torch.tensor(excl))
    counts = allowed.sum(dim=1)
    assert set(counts.tolist()) == {16, 32}
    j, dcol = torch.meshgrid(torch.arange(n), torch.arange(c), indexing="ij")
    v = ((7 * j + 3 * dcol + (j * dcol) % 5) % 8 + 1).float().unsqueeze(0)
    o_want = (allowed.double() @ v[0].double() / counts.double().unsqueeze(1)).float()
    zeros = torch.zeros(1, n, c)
    got = run_attention(hip_lib, lib, 1, n, 1, False, q, k, v, zeros, (zeros, zeros, zeros), scale=0.125)
    assert torch.equal(got[0][0], o_want), "O is not the exact mean of V over the allowed keys"
    lse_want = counts.double().log()
    assert float((got[1][0, 0].double() - lse_want).abs().max()) < 1e-6
    # the fp32 entry on the same data, so that a mistake in this test's own arithmetic shows as such
    got32 = run_attention(hip_lib, lib, 1, n, 1, False, q, k, v, zeros, (zeros, zeros, zeros), sfx="", scale=0.125)
    assert torch.equal(got32[0][0], o_want)


def test_gradient_scale_invariance(hip_lib):
    from gaia_seg_amd.hip import lib
    b, n, heads = 2, 129, 3
    q, k, v, do, bq, bk, bv = U.attention_inputs(b, n, heads, False, SEED)
    run = lambda g, vv=v, qq=q, kk=k: run_attention(hip_lib, lib, b, n, heads, False, qq, kk, vv, g,   # noqa: E731
                                                    (bq, bk, bv))[2:5]
    base = run(do)
    for e in (-20, 12):
        f = 2.0 ** e
        for nm, t, u in zip(NAMES[2:5], run(do * f), base):
            assert torch.equal(t, u * f), "%s at dO x 2^%d is not 2^%d x the gradient at dO" % (nm, e, e)
    for nm, t in zip(NAMES[2:5], run(torch.zeros_like(do))):
        assert not bool(t.any()), "%s: dO == 0 must give exact zeros" % nm
    # a one-hot P (every query's last-key score is 30 above the rest) and |V| up to 30
    qd, kd = U.attention_inputs(b, n, heads, True, SEED)[:2]
    qd[:, :, ::U.HEAD_DIM] = 8.0
    vbig = (v * 10).clamp(-30, 30)
    vbig[:, -1, :8] = 30.0
    for nm, t in zip(NAMES[2:5], run(do, vbig, qd, kd)):
        assert bool(torch.isfinite(t).all()), "%s: not finite at |V| = 30" % nm


def run_relpos(L, lib, b, wh, ww, heads, sliced, q, k, v, table):
    return A.run_relpos(L, lib, b, wh, ww, heads, sliced, q, k, v, table, sfx="_f16")


F16_RELPOS_CASES = [RELPOS_CASES[0], RELPOS_CASES[1], RELPOS_CASES[3]]   # 2x3, crosses a key tile, N > 128


@pytest.mark.parametrize("case", F16_RELPOS_CASES, ids=[c[0] for c in F16_RELPOS_CASES])
def test_relpos_attention_f16_forward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, wh, ww, heads, sliced, _ = case
    n = wh * ww + 1
    q, k, v = U.attention_inputs(b, n, heads, False, 7)[:3]
    zero = torch.zeros((2 * wh - 1) * (2 * ww - 1) + 3, heads)
    plain = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, None)
    for nm, t, u in zip(("O", "lse"), run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, zero), plain):
        assert torch.equal(t, u), "%s: a zero table changes bits" % nm
    table = make_table(wh, ww, heads, False, 11)
    ref = B.relpos_attention(q.double(), k.double(), v.double(), heads, table.double(), wh, ww)
    bias = table.double()[B.relpos_index(wh, ww)].permute(2, 0, 1)
    wit = W.witness(q, k, v, None, heads, bias=bias)
    first = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, table)
    second = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, table)
    for nm, t, u in zip(("O", "lse"), first, second):
        assert torch.equal(t, u), "%s differs between two runs" % nm
    assert rel_err(plain[0], ref[0]) > 1e-2, "the table does not change O enough to be seen"
    check_budget(name, ("O", "lse"), first, wit, ref)


def test_attention_f16_argument_checks(hip_lib):
    """each documented error code of the four entries, and the outputs still hold the sentinel afterwards"""
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    b, n, heads, c = 1, 7, 2, 128
    x = torch.zeros(b, n, c, device=DEV)
    out = [torch.full((b, n, c), SENTINEL, device=DEV) for _ in range(4)]
    lse = torch.full((b * heads * n,), SENTINEL, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    table = torch.zeros(18, heads, device=DEV)
    p = x.data_ptr()

    def fwd(d, q=p, k=p, v=p, o=out[0].data_ptr(), l=lse.data_ptr()):
        return L.gs_attention_forward_f16(ctypes.byref(d) if d is not None else None, q, k, v, o, l, st)

    def rel(d, q=p, t=table.data_ptr(), ldt=heads, wh=2, ww=3, o=out[0].data_ptr()):
        return L.gs_attention_relpos_forward_f16(ctypes.byref(d) if d is not None else None, q, p, p, t, ldt, wh, ww,
                                                 o, lse.data_ptr(), st)

    def bwd(d, dq=out[1].data_ptr(), wsp=ws.data_ptr(), wsb=4096, o=p):
        return L.gs_attention_backward_f16(ctypes.byref(d) if d is not None else None, p, p, p, o, lse.data_ptr(),
                                           p, dq, out[2].data_ptr(), out[3].data_ptr(), 0, wsp, wsb, st)

    def desc(**kw):
        d = lib.attention_desc(b, n, heads, U.SCALE)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    good = desc()
    need = L.gs_attention_workspace_bytes_f16(ctypes.byref(good))
    assert need >= 4 * b * heads * (n + 1) and need % 16 == 0
    assert fwd(None) == GS_E_NULL and bwd(None) == GS_E_NULL and rel(None) == GS_E_NULL
    assert fwd(good, q=None) == GS_E_NULL and fwd(good, o=None) == GS_E_NULL and fwd(good, l=None) == GS_E_NULL
    assert rel(good, t=None) == GS_E_NULL and rel(good, q=None) == GS_E_NULL
    assert bwd(good, dq=None) == GS_E_NULL and bwd(good, wsp=None) == GS_E_NULL
    for bad in (desc(B=0), desc(N=0), desc(heads=0), desc(N=-3), desc(scale=0.0), desc(scale=-1.0),
                desc(ldq=c - 4), desc(ldo=64), desc(lddk=c - 4)):
        assert fwd(bad) == GS_E_BADARG and bwd(bad) == GS_E_BADARG and rel(bad) == GS_E_BADARG
        assert L.gs_attention_workspace_bytes_f16(ctypes.byref(bad)) == 0
    for bad in (desc(ldk=c + 2), desc(lddv=c + 1)):
        assert fwd(bad) == GS_E_ALIGN and bwd(bad) == GS_E_ALIGN and rel(bad) == GS_E_ALIGN
        assert L.gs_attention_workspace_bytes_f16(ctypes.byref(bad)) == 0
    assert rel(good, wh=3) == GS_E_BADARG and rel(good, ldt=1) == GS_E_BADARG and rel(good, ww=0) == GS_E_BADARG
    assert fwd(good, q=p + 4) == GS_E_ALIGN and fwd(good, o=out[0].data_ptr() + 8) == GS_E_ALIGN
    assert rel(good, q=p + 4) == GS_E_ALIGN and rel(good, t=table.data_ptr() + 2) == GS_E_ALIGN
    assert bwd(good, dq=out[1].data_ptr() + 4) == GS_E_ALIGN and bwd(good, wsp=ws.data_ptr() + 4) == GS_E_ALIGN
    assert bwd(good, wsb=need - 1) == GS_E_WORKSPACE and bwd(good, wsb=0) == GS_E_WORKSPACE
    assert L.gs_attention_workspace_bytes_f16(None) == 0
    torch.cuda.synchronize()
    for t in out + [lse]:
        assert bool((t == SENTINEL).all()), "a refused call wrote to an output"


class Counter:
    """counts the calls of the bound attention entries; restores them on exit"""
    NAMES = tuple("gs_attention_%s%s" % (w, s) for w in ("forward", "backward", "relpos_forward")
                  for s in ("", "_f16"))

    def __init__(self, L):
        self.L, self.calls, self.saved = L, {n: 0 for n in self.NAMES}, {}

    def __enter__(self):
        for name in self.NAMES:
            fn = self.saved[name] = getattr(self.L, name)

            def counted(*a, _fn=fn, _name=name):
                self.calls[_name] += 1
                return _fn(*a)
            setattr(self.L, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.L, name, fn)
        return False

    def used(self):
        return {k[len("gs_attention_"):]: v for k, v in self.calls.items() if v}


def test_ops_attention_dispatch(hip_lib):
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    b, n, heads = 2, 17, 1
    q, k, v, do = U.attention_inputs(b, n, heads, False, SEED)[:4]

    def run(f16):
        tape = Tape()
        acts = [Act(t.view(b, 1, n, -1).contiguous().to(DEV)) for t in (q, k, v)]
        for a in acts:
            a.requires_grad = True
        out = ops.attention(tape, *acts, heads, U.SCALE, f16=f16)
        out.g = do.view(b, 1, n, -1).contiguous().to(DEV)
        tape.backward()
        torch.cuda.synchronize()
        return [out.t.cpu()] + [a.g.cpu() for a in acts]

    with Counter(hip_lib) as cnt:
        plain, flagged = run(False), run(True)
    assert cnt.used() == {"forward": 2, "backward": 2}, cnt.used()
    for t, u in zip(plain, flagged):
        assert torch.equal(t, u), "f16=True outside an fp16 mode changed bits"
    with ops.train_precision("fp16"):
        with Counter(hip_lib) as cnt:
            off = run(False)
        assert cnt.used() == {"forward": 1, "backward": 1}, cnt.used()
        with Counter(hip_lib) as cnt:
            on = run(True)
        assert cnt.used() == {"forward_f16": 1, "backward_f16": 1}, cnt.used()
    for t, u in zip(plain, off):
        assert torch.equal(t, u)
    ref = U.attention_ref(q, k, v, do, heads)
    assert 1e-4 < rel_err(on[0].view(b, n, -1), ref[0]) < 1e-2
    assert math.isfinite(float(on[1].abs().max()))
