"""gs_attention_* and gs_vit_tokens_* through the C-ABI (csrc/attention.hip), under the protocol of
tests/test_convnext_ops_gpu.py:

  * outputs are pre-filled with a sentinel: everything outside the written slice -- pad columns of a wide
    pitch, the columns of an inactive head, the neighbours of a column slice -- must still hold it;
  * pad columns and inactive head columns of the inputs hold NaN;
  * workspaces are exactly the queried size, hold NaN (0xFF), and sit in front of a 4 KiB guard;
  * every case runs twice and the two results are bit-identical (fixed summation order, no atomics);
  * TOL = 3e-5 in conftest.rel_err against float64, that file's bound for fp32 operators.

The cases are placed relative to T = 128 (tests/util_vit.py), the larger of the kernels' two tiles: a
workgroup owns 128 query rows (keys in the dK / dV kernel) and sweeps the other operand in tiles of 32
rows.  tests/test_elastic_vit.py checks on the CPU that float32 torch stays below 1e-5 on these inputs, so
the bound here is a statement about the kernels.  The harness (run_attention, Workspace, active, ...) is
tests/util_attention_gpu.py, shared with the fp16-operand and the relative-position tests."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_attention_gpu as A
import util_vit as U
from util_attention_gpu import (DEV, GS_E_ALIGN, GS_E_BADARG, GS_E_NULL, GS_E_WORKSPACE, NAN, SENTINEL, active, padded,
                                run_attention, stream)

pytestmark = pytest.mark.gpu
TOL = 3e-5
PARENT_BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_parent_bits.json")


@pytest.mark.parametrize("case", U.ATTENTION_CASES, ids=[c[0] for c in U.ATTENTION_CASES])
def test_attention_forward_backward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, n, heads, sliced, dominant = case
    q, k, v, do, bq, bk, bv = U.attention_inputs(b, n, heads, dominant, 5)
    o_r, lse_r, dq_r, dk_r, dv_r = U.attention_ref(q, k, v, do, heads)
    want = (o_r, lse_r, dq_r, dk_r, dv_r, dq_r + bq.double(), dk_r + bk.double(), dv_r + bv.double())
    names = ("O", "lse", "dQ", "dK", "dV", "dQ+", "dK+", "dV+")
    first = run_attention(hip_lib, lib, b, n, heads, sliced, q, k, v, do, (bq, bk, bv))
    second = run_attention(hip_lib, lib, b, n, heads, sliced, q, k, v, do, (bq, bk, bv))
    errs = {nm: rel_err(g, r) for nm, g, r in zip(names, first, want)}
    print(name, {nm: "%.2e" % e for nm, e in errs.items()})
    for nm, a, bb in zip(names, first, second):
        assert torch.equal(a, bb), "%s differs between two runs" % nm
    if n == 1:   # softmax of one element: O = V, and dP == delta bit for bit
        assert torch.equal(first[0], v), "single token: O != V"
        assert torch.equal(first[4], do), "single token: dV != dO"
        assert not bool(first[2].any()) and not bool(first[3].any()), "single token: dQ, dK must be exactly 0"
        names, first, want = names[:2] + names[4:], first[:2] + first[4:], want[:2] + want[4:]
    for nm, g, r in zip(names, first, want):
        assert rel_err(g, r) < TOL, "%s: rel_err %.3g" % (nm, rel_err(g, r))


def test_attention_argument_checks(hip_lib):
    """each documented error code, and the outputs still hold the sentinel afterwards"""
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    b, n, heads, c = 1, 5, 2, 128
    x = torch.zeros(b, n, c, device=DEV)
    out = [torch.full((b, n, c), SENTINEL, device=DEV) for _ in range(4)]
    lse = torch.full((b * heads * n,), SENTINEL, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = x.data_ptr()

    def fwd(d, q=p, k=p, v=p, o=out[0].data_ptr(), l=lse.data_ptr()):
        return L.gs_attention_forward(ctypes.byref(d) if d is not None else None, q, k, v, o, l, st)

    def bwd(d, dq=out[1].data_ptr(), wsp=ws.data_ptr(), wsb=4096, o=p):
        return L.gs_attention_backward(ctypes.byref(d) if d is not None else None, p, p, p, o, lse.data_ptr(), p,
                                       dq, out[2].data_ptr(), out[3].data_ptr(), 0, wsp, wsb, st)

    def desc(**kw):
        d = lib.attention_desc(b, n, heads, U.SCALE)
        for key, val in kw.items():
            setattr(d, key, val)
        return d

    good = desc()
    need = L.gs_attention_workspace_bytes(ctypes.byref(good))
    assert need >= 4 * b * heads * n
    assert fwd(None) == GS_E_NULL and bwd(None) == GS_E_NULL
    assert fwd(good, q=None) == GS_E_NULL and fwd(good, o=None) == GS_E_NULL and fwd(good, l=None) == GS_E_NULL
    assert bwd(good, dq=None) == GS_E_NULL and bwd(good, wsp=None) == GS_E_NULL
    for bad in (desc(B=0), desc(N=0), desc(heads=0), desc(N=-3), desc(scale=0.0), desc(scale=-1.0),
                desc(ldq=c - 4), desc(ldo=64), desc(lddk=c - 4)):
        assert fwd(bad) == GS_E_BADARG and bwd(bad) == GS_E_BADARG
        assert L.gs_attention_workspace_bytes(ctypes.byref(bad)) == 0
    for bad in (desc(ldk=c + 2), desc(lddv=c + 1)):
        assert fwd(bad) == GS_E_ALIGN and bwd(bad) == GS_E_ALIGN
        assert L.gs_attention_workspace_bytes(ctypes.byref(bad)) == 0
    assert fwd(good, q=p + 4) == GS_E_ALIGN and fwd(good, o=out[0].data_ptr() + 8) == GS_E_ALIGN
    assert bwd(good, dq=out[1].data_ptr() + 4) == GS_E_ALIGN and bwd(good, wsp=ws.data_ptr() + 4) == GS_E_ALIGN
    assert bwd(good, wsb=need - 1) == GS_E_WORKSPACE and bwd(good, wsb=0) == GS_E_WORKSPACE
    assert L.gs_attention_workspace_bytes(None) == 0
    torch.cuda.synchronize()
    for t in out + [lse]:
        assert bool((t == SENTINEL).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("precision", list(A.PRECISIONS))
@pytest.mark.parametrize("kind,case", A.BITS_CASES, ids=["%s-%s" % (k, c[0]) for k, c in A.BITS_CASES])
def test_attention_matches_parent_bits(hip_lib, kind, case, precision):
    """Every output of the attention entries, bit for bit, against tests/golden/attention_parent_bits.json:
    SHA-256 digests recorded on an MI355X with the library of the commit before the fp32 and the fp16-operand
    kernels became one template per kernel over the operand format (csrc/attention_common.h).  A refactor of
    these kernels keeps every bit; a change that is meant to move them regenerates the file with
    tests/golden/make_attention_parent_bits.py, whose docstring says how."""
    from gaia_seg_amd.hip import lib
    with open(PARENT_BITS) as f:
        want = json.load(f)["%s/%s/%s" % (kind, case[0], precision)]
    got = A.output_digests(hip_lib, lib, kind, case, precision)
    assert sorted(got) == sorted(want)
    differ = [nm for nm in got if got[nm] != want[nm]]
    assert not differ, "%s %s %s: %s differ from the parent's bits" % (kind, case[0], precision, differ)


def run_tokens(L, lib, b, t, d, n_max, d_max, patches, cls, pos, dx):
    st = stream()
    ldp = d + 4
    pg = padded(patches, ldp, NAN)
    cg = padded(cls, d_max, NAN)
    eg = torch.full((n_max, d_max), NAN)
    eg[:t + 1, :d] = pos
    eg = eg.to(DEV)
    x = torch.full((b, t + 1, d_max), SENTINEL, device=DEV)
    lib.check(L.gs_vit_tokens_forward(pg.data_ptr(), ldp, cg.data_ptr(), eg.data_ptr(), d_max, x.data_ptr(), d_max,
                                      b, t, d, st), "tokens fwd")
    dxg = padded(dx, d_max, NAN)
    dp = torch.full((b, t, ldp), SENTINEL, device=DEV)
    dc = torch.full((d_max,), SENTINEL, device=DEV)
    de = torch.full((n_max, d_max), SENTINEL, device=DEV)
    lib.check(L.gs_vit_tokens_backward(dxg.data_ptr(), d_max, dp.data_ptr(), ldp, dc.data_ptr(), de.data_ptr(),
                                       d_max, b, t, d, st), "tokens bwd")
    torch.cuda.synchronize()
    de_cpu = de.cpu()
    assert bool((de_cpu[t + 1:] == SENTINEL).all()), "dpos: a store to a row past the active tokens"
    return (active(x, 0, d, "x"), active(dp, 0, d, "dpatches"), active(dc, 0, d, "dcls"),
            active(de[:t + 1], 0, d, "dpos"))


def test_vit_tokens(hip_lib):
    from gaia_seg_amd.hip import lib
    b, t, d, n_max, d_max = 2, 6, 8, 12, 12
    g = torch.Generator().manual_seed(3)
    patches, cls, pos, dx = (torch.randn(*s, generator=g) for s in ((b, t, d), (d,), (t + 1, d), (b, t + 1, d)))
    want = U.tokens_ref(patches, cls, pos, dx)
    first = run_tokens(hip_lib, lib, b, t, d, n_max, d_max, patches, cls, pos, dx)
    second = run_tokens(hip_lib, lib, b, t, d, n_max, d_max, patches, cls, pos, dx)
    for name, a, bb, r in zip(("x", "dpatches", "dcls", "dpos"), first, second, want):
        assert torch.equal(a, bb), "%s differs between two runs" % name
        assert rel_err(a, r) < TOL, "%s: rel_err %.3g" % (name, rel_err(a, r))
    # argument checks
    L, st, p = hip_lib, stream(), torch.zeros(64, device=DEV).data_ptr()
    assert L.gs_vit_tokens_forward(None, 8, p, p, 8, p, 8, 1, 1, 8, st) == GS_E_NULL
    assert L.gs_vit_tokens_forward(p, 8, p, p, 8, p, 8, 0, 1, 8, st) == GS_E_BADARG
    assert L.gs_vit_tokens_forward(p, 4, p, p, 8, p, 8, 1, 1, 8, st) == GS_E_BADARG
    assert L.gs_vit_tokens_forward(p, 8, p, p, 8, p, 8, 1, 1, 6, st) == GS_E_ALIGN
    assert L.gs_vit_tokens_forward(p, 8, p, p, 8, p + 4, 8, 1, 1, 8, st) == GS_E_ALIGN
    assert L.gs_vit_tokens_backward(p, 8, p, 8, None, p, 8, 1, 1, 8, st) == GS_E_NULL
    assert L.gs_vit_tokens_backward(p, 8, p, 8, p, p, 4, 1, 1, 8, st) == GS_E_BADARG
    assert L.gs_vit_tokens_backward(p, 10, p, 8, p, p, 8, 1, 1, 8, st) == GS_E_ALIGN


def test_bilinear_downsample_matches_interpolate():
    """ops.bilinear towards a smaller size (the neck's 0.5 level) against F.interpolate(scale_factor=0.5),
    forward and adjoint"""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(2, 8, 6, 10, generator=g), torch.randn(2, 8, 3, 5, generator=g)
    xr = x.double().requires_grad_(True)
    y_r = F.interpolate(xr, scale_factor=0.5, mode="bilinear", align_corners=False)
    y_r.backward(dy.double())
    tape = Tape()
    a = Act(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    out = ops.bilinear(tape, a, (3, 5))
    out.g = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(out.t.permute(0, 3, 1, 2), y_r) < TOL
    assert rel_err(a.g.permute(0, 3, 1, 2), xr.grad) < TOL
