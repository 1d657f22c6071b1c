"""SegNeXt's multi-scale convolutional attention and its gate through the C-ABI (gs_msca_forward /
_backward, gs_gate_mul_forward / _backward; csrc/msca.hip), under the protocol of tests/test_dwconv_gpu.py.

Every case runs on buffers that forgive nothing:

  * outputs (s, dx, the 14 parameter gradients, y, dg, du) are pre-filled with a sentinel: everything
    outside the written slice -- pad columns of a wide pitch, the neighbours of a concat slice, filter
    channels C .. C_ld-1 -- must still hold it afterwards;
  * pad columns of x and ds beyond C, and filter and bias channels beyond C, hold NaN;
  * the saved buffer and the workspace are exactly gs_msca_saved_bytes(d) / gs_msca_workspace_bytes(d)
    bytes of NaN (0xFF) in front of a 4 KiB guard with a known byte pattern;

and with two kinds of data:

  (a) exact: x, ds, every filter and every bias drawn from {-1, +1}.  Every forward value, data gradient,
      filter gradient and bias gradient is then an integer below 2^24 up to 16384 pixels (|s| <= 15954,
      |da| <= 612, |d w0| <= 612 P, |d w_col21|, |d w_row21| <= 547 P), so fp32 accumulation is exact
      in any order: torch.equal against float64.  The test asserts the bound itself, by running the float64
      reference on absolute values (all-ones data of the same shapes): its maximum must stay below 2^24.
  (b) random: standard normal data against the float64 reference within TOL = 3e-5 (rel_err, that file's
      bound for fp32 operators), run twice and bit-identical (fixed reduction order, no atomics).

The reference is the chain as seven F.conv2d(groups=C) calls and three adds in float64 with autograd.  Each
case runs the forward, the backward with accumulate = 0 and the backward with accumulate = 1 onto a base."""
import ctypes
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5
SENTINEL = 7.0
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
NAN = float("nan")
K0, KS = 5, (7, 11, 21)
NAMES = ("w0", "b0", "w_row0", "w_row1", "w_row2", "b_row0", "b_row1", "b_row2",
         "w_col0", "w_col1", "w_col2", "b_col0", "b_col1", "b_col2")


class MCase(NamedTuple):
    n: int
    h: int
    w: int
    c: int
    c_max: Optional[int] = None    # filter channels (C_ld)
    ldx: Optional[int] = None
    lds: Optional[int] = None      # width of the buffer s / ds is a slice of
    s_c0: int = 0                  # first channel of that slice

    def id(self):
        s = "%dx%dx%dx%d" % (self.n, self.h, self.w, self.c)
        if self.c_max:
            s += "-of%d" % self.c_max
        if self.ldx:
            s += "-ldx%d" % self.ldx
        if self.lds:
            s += "-slice%dof%d" % (self.s_c0, self.lds)
        return s


CASES = [
    MCase(1, 1, 1, 4),                       # centre taps only
    MCase(2, 5, 7, 8),                       # the map is smaller than every strip's reach
    MCase(1, 3, 40, 8),                      # one direction longer than 21, the other shorter than 5
    MCase(1, 40, 3, 8),
    MCase(1, 33, 17, 12),                    # odd sizes across tile edges
    MCase(2, 9, 11, 20, c_max=32, ldx=24),   # a sliced filter and a wide pitch
    MCase(2, 9, 11, 8, lds=24, s_c0=8),      # s / ds as slice 8..16 of a 24-wide buffer
    MCase(2, 8, 8, 320),                     # many channel blocks
    MCase(2, 24, 40, 8),                     # 1920 pixels, several filter-gradient runs
    MCase(2, 64, 128, 8),                    # 16384 pixels, multi-stage reduce
]


def filter_shapes(c):
    """the 14 parameters in the order of gs_msca_filters, channels last"""
    return ([(K0, K0, c), (c,)] + [(k, c) for k in KS] + [(c,)] * 3 + [(k, c) for k in KS] + [(c,)] * 3)


def make_data(c, kind, seed):
    """x, ds, base [n,h,w,c] and the 14 parameters; kind: 'pm1' (+-1), 'ones' or 'normal'"""
    gen = torch.Generator().manual_seed(seed)
    if kind == "pm1":
        draw = lambda *s: (torch.randint(0, 2, s, generator=gen) * 2 - 1).float()    # noqa: E731
    elif kind == "ones":
        draw = lambda *s: torch.ones(*s)    # noqa: E731
    else:
        draw = lambda *s: torch.randn(*s, generator=gen)    # noqa: E731
    shape = (c.n, c.h, c.w, c.c)
    return draw(*shape), draw(*shape), draw(*shape), [draw(*s) for s in filter_shapes(c.c)]


def reference(c, x, ds, params):
    """float64 on the CPU: s, dx [n,h,w,c] and the 14 gradients in the layouts of make_data"""
    C = c.c
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in params]
    w0, b0, wrow, brow, wcol, bcol = ps[0], ps[1], ps[2:5], ps[5:8], ps[8:11], ps[11:14]
    a = F.conv2d(xr, w0.permute(2, 0, 1).unsqueeze(1), b0, padding=K0 // 2, groups=C)
    s = a
    for i, k in enumerate(KS):
        r = F.conv2d(a, wrow[i].t().reshape(C, 1, 1, k), brow[i], padding=(0, k // 2), groups=C)
        s = s + F.conv2d(r, wcol[i].t().reshape(C, 1, k, 1), bcol[i], padding=(k // 2, 0), groups=C)
    s.backward(ds.double().permute(0, 3, 1, 2))
    return (s.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous(),
            [p.grad for p in ps])


def padded(t, ld, fill, c0=0):
    """t [..., c] inside a [..., ld] buffer filled with ``fill``, at channel c0"""
    buf = torch.full(t.shape[:-1] + (ld,), fill)
    buf[..., c0:c0 + t.shape[-1]] = t
    return buf.to(DEV)


def active(buf, c0, c, what):
    """synchronise; everything outside [..., c0:c0+c] still holds the sentinel; the slice on the CPU"""
    torch.cuda.synchronize()
    out = buf.cpu()
    outside = torch.ones_like(out, dtype=torch.bool)
    outside[..., c0:c0 + c] = False
    assert bool((out[outside] == SENTINEL).all()), "%s: a store outside the active slice" % what
    got = out[..., c0:c0 + c].contiguous()
    assert bool(torch.isfinite(got).all()), "%s: NaN -- a pad column or an unwritten partial was read" % what
    return got


def guarded(need):
    buf = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
    buf[:need] = 0xFF
    buf[need:] = GUARD_BYTE
    return buf


def table(lib, ts):
    p = [t.data_ptr() for t in ts]
    return lib.msca_filters(p[0], p[1], p[2:5], p[5:8], p[8:11], p[11:14])


def run_all(hip_lib, lib, c, x, ds, base, params):
    """forward, backward (overwrite), backward (accumulate onto base): s, dx, dx+, and the 14 gradients of
    both backward calls"""
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    c_ld, ldx, lds = c.c_max or c.c, c.ldx or c.c, c.lds or c.c
    d = lib.msca_desc(c.n, c.h, c.w, c.c, c_ld=c_ld, ldx=ldx, lds=lds, k0=K0, k=KS)
    db, st = ctypes.byref(d), current_stream_ptr()
    xg, dsg = padded(x, ldx, NAN), padded(ds, lds, NAN, c.s_c0)
    pg = [padded(p, c_ld, NAN) for p in params]
    off = 4 * c.s_c0
    f = table(lib, pg)
    need_saved, need_ws = hip_lib.gs_msca_saved_bytes(db), hip_lib.gs_msca_workspace_bytes(db)
    assert need_saved == 4 * c.n * c.h * c.w * c.c * 4 and need_ws > 0
    saved = guarded(need_saved)
    s = torch.full((c.n, c.h, c.w, lds), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_msca_forward(db, xg.data_ptr(), ctypes.byref(f), s.data_ptr() + off, saved.data_ptr(),
                                      st), "fwd")
    outs = [active(s, c.s_c0, c.c, "s")]
    grads = []
    for acc, dx in ((0, torch.full((c.n, c.h, c.w, ldx), SENTINEL, device=DEV)), (1, padded(base, ldx, SENTINEL))):
        ws = guarded(need_ws)
        gg = [torch.full(p.shape, SENTINEL, device=DEV) for p in pg]
        g = table(lib, gg)
        lib.check(hip_lib.gs_msca_backward(db, xg.data_ptr(), dsg.data_ptr() + off, ctypes.byref(f), saved.data_ptr(),
                                           dx.data_ptr(), acc, ctypes.byref(g), ws.data_ptr(), need_ws, st),
                  "bwd acc=%d" % acc)
        outs.append(active(dx, 0, c.c, "dx acc=%d" % acc))
        grads.append([active(t, 0, c.c, "d %s acc=%d" % (n, acc)) for n, t in zip(NAMES, gg)])
        assert bool((ws[need_ws:] == GUARD_BYTE).all()), "the backward overran the workspace"
    assert bool((saved[need_saved:] == GUARD_BYTE).all()), "the forward overran the saved buffer"
    return outs, grads


def compare_exact(name, got, ref):
    assert torch.equal(got.double(), ref), "exact leg, %s: %d of %d elements differ, largest by %g" % (
        name, int((got.double() != ref).sum()), ref.numel(), float((got.double() - ref).abs().max()))


@pytest.mark.parametrize("case", CASES, ids=MCase.id)
def test_msca_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    c = case
    # the bound of the exact leg: the reference on absolute values
    x1, ds1, _, p1 = make_data(c, "ones", 0)
    s_b, dx_b, g_b = reference(c, x1, ds1, p1)
    bound = max(float(t.abs().max()) for t in [s_b, dx_b + 1] + g_b)
    print("%s: exact leg, bound %g" % (c.id(), bound))
    assert bound < 2 ** 24
    # (a) exact
    x, ds, base, params = make_data(c, "pm1", 11)
    s_r, dx_r, g_r = reference(c, x, ds, params)
    outs, grads = run_all(hip_lib, lib, c, x, ds, base, params)
    for name, got, ref in zip(("s", "dx", "dx+"), outs, (s_r, dx_r, dx_r + base.double())):
        compare_exact(name, got, ref)
    for acc in (0, 1):
        for name, got, ref in zip(NAMES, grads[acc], g_r):
            compare_exact("d %s (accumulate %d)" % (name, acc), got, ref)
    # (b) random, twice
    x, ds, base, params = make_data(c, "normal", 12)
    s_r, dx_r, g_r = reference(c, x, ds, params)
    first = run_all(hip_lib, lib, c, x, ds, base, params)
    second = run_all(hip_lib, lib, c, x, ds, base, params)
    for name, a, b, ref in zip(("s", "dx", "dx+"), first[0], second[0], (s_r, dx_r, dx_r + base.double())):
        err = rel_err(a, ref)
        print("%s: random leg, %s rel_err %.3g" % (c.id(), name, err))
        assert err < TOL, name
        assert torch.equal(a, b), "%s: two runs of the same input differ" % name
    for acc in (0, 1):
        for name, a, b, ref in zip(NAMES, first[1][acc], second[1][acc], g_r):
            err = rel_err(a, ref)
            print("%s: random leg, d %s (accumulate %d) rel_err %.3g" % (c.id(), name, acc, err))
            assert err < TOL, name
            assert torch.equal(a, b), "d %s: two runs of the same input differ" % name


GATE_CASES = [(1, 4, None), (77, 20, 24), (4096, 64, None)]


def run_gate(hip_lib, lib, rows, c, ld, g, u, dy, base):
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    st = current_stream_ptr()
    gg, ug, dyg = padded(g, ld, NAN), padded(u, ld, NAN), padded(dy, ld, NAN)
    y = torch.full((rows, ld), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_gate_mul_forward(gg.data_ptr(), ug.data_ptr(), y.data_ptr(), rows, c, ld, ld, ld, st),
              "gate fwd")
    outs = [active(y, 0, c, "y")]
    for acc, du in ((0, torch.full((rows, ld), SENTINEL, device=DEV)), (1, padded(base, ld, SENTINEL))):
        dg = torch.full((rows, ld), SENTINEL, device=DEV)
        lib.check(hip_lib.gs_gate_mul_backward(dyg.data_ptr(), gg.data_ptr(), ug.data_ptr(), dg.data_ptr(),
                                               du.data_ptr(), rows, c, ld, ld, ld, ld, ld, acc, st), "gate bwd")
        outs += [active(dg, 0, c, "dg acc=%d" % acc), active(du, 0, c, "du acc=%d" % acc)]
    return outs


@pytest.mark.parametrize("rows,c,ld", GATE_CASES, ids=["1x4", "77x20-ld24", "4096x64"])
def test_gate_mul_kernels(hip_lib, rows, c, ld):
    from gaia_seg_amd.hip import lib
    ld = ld or c
    for kind, seed in (("pm1", 21), ("normal", 22)):
        gen = torch.Generator().manual_seed(seed)
        if kind == "pm1":
            draw = lambda: (torch.randint(0, 2, (rows, c), generator=gen) * 2 - 1).float()    # noqa: E731
        else:
            draw = lambda: torch.randn(rows, c, generator=gen)    # noqa: E731
        g, u, dy, base = draw(), draw(), draw(), draw()
        gd, ud, dyd = g.double(), u.double(), dy.double()
        want = (gd * ud, dyd * ud, dyd * gd, dyd * ud, dyd * gd + base.double())
        first = run_gate(hip_lib, lib, rows, c, ld, g, u, dy, base)
        second = run_gate(hip_lib, lib, rows, c, ld, g, u, dy, base)
        for name, a, b, ref in zip(("y", "dg", "du", "dg (accumulate)", "du+"), first, second, want):
            if kind == "pm1":
                compare_exact(name, a, ref)
            else:
                assert rel_err(a, ref) < TOL, name
            assert torch.equal(a, b), "%s: two runs of the same input differ" % name
