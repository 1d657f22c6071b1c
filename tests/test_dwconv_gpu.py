"""The depthwise 3x3 convolution through the C-ABI (gs_dwconv2d_forward / _dgrad / _wgrad;
csrc/dwconv.hip), under the protocol of tests/test_wgrad_gpu.py.

Every case runs on buffers that forgive nothing:

  * outputs (y, dx, dw) are pre-filled with a sentinel: everything outside the written slice -- pad
    columns of a wide pitch, the neighbours of a concat slice, weight channels C .. C_ld-1 -- must still
    hold it afterwards;
  * pad columns of x and dy beyond C, and weight channels beyond C, hold NaN;
  * the weight-gradient workspace is exactly gs_dwconv2d_workspace_bytes(d) bytes of NaN (0xFF) in front
    of a 4 KiB guard with a known byte pattern;

and with two kinds of data:

  (a) exact: nonzero integers in {+-1, +-2, +-3}.  Every product and partial sum is an integer below
      2^24 (largest |dw| here: 9 * 16384), so fp32 accumulation is exact in any order: torch.equal
      against float64.  One dropped, duplicated or misplaced pixel or tap moves an element by >= 1.
  (b) random: standard normal data against the float64 reference within TOL = 3e-5 (that file's bound
      for fp32 operators), run twice and bit-identical (fixed reduction order, no atomics)."""
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


class DCase(NamedTuple):
    n: int
    h: int
    w: int
    c: int
    dil: int = 1
    pad: Optional[int] = None      # default: dil ('same')
    c_max: Optional[int] = None    # weight channels (C_ld)
    ldx: Optional[int] = None
    ldy: Optional[int] = None      # width of the buffer y / dy is a slice of
    y_c0: int = 0                  # first channel of that slice

    def id(self):
        s = "%dx%dx%dx%d-d%d" % (self.n, self.h, self.w, self.c, self.dil)
        if self.pad is not None:
            s += "-p%d" % self.pad
        if self.c_max:
            s += "-of%d" % self.c_max
        if self.ldx:
            s += "-ldx%d" % self.ldx
        if self.ldy:
            s += "-slice%dof%d" % (self.y_c0, self.ldy)
        return s


CASES = [
    DCase(2, 9, 11, 8),                                  # plain
    DCase(1, 1, 1, 4),                                   # single pixel: centre tap only
    DCase(2, 5, 7, 20, dil=6, c_max=32, ldx=24),         # dilation larger than the map; sliced weight; wide pitch
    DCase(1, 33, 17, 12, dil=2),                         # odd sizes across tile edges; 561 pixels in the wgrad reduce
    DCase(2, 16, 64, 64, dil=12),                        # dilation between H and W
    DCase(2, 8, 8, 320),                                 # many channel blocks
    DCase(2, 64, 128, 8, dil=3),                         # 16384 pixels: multi-stage wgrad reduce
    DCase(2, 9, 11, 8, ldy=24, y_c0=8),                  # concat-slice destination, neighbours untouched
    # beyond 'same' padding: a smaller output, and padding wider than the taps reach (the data
    # gradient's mirrored stencil then has a negative padding)
    DCase(2, 9, 11, 8, dil=2, pad=1),
    DCase(1, 6, 7, 8, dil=1, pad=3),
]


def geom(c):
    pad = c.dil if c.pad is None else c.pad
    ho, wo = c.h + 2 * pad - 2 * c.dil, c.w + 2 * pad - 2 * c.dil
    return pad, ho, wo, c.c_max or c.c, c.ldx or c.c, c.ldy or c.c


def make_desc(lib, c):
    pad, _, _, c_ld, ldx, ldy = geom(c)
    return lib.dwconv_desc(c.n, c.h, c.w, c.c, pad, c.dil, c_ld=c_ld, ldx=ldx, ldy=ldy)


def small_ints(gen, *shape):
    return (torch.randint(1, 4, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def make_data(c, exact, seed):
    """x [n,h,w,c], w [3,3,c], dy [n,ho,wo,c], base (the dx an accumulating dgrad adds to)"""
    _, ho, wo, _, _, _ = geom(c)
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda *s: small_ints(gen, *s)) if exact else (lambda *s: torch.randn(*s, generator=gen))
    return draw(c.n, c.h, c.w, c.c), draw(3, 3, c.c), draw(c.n, ho, wo, c.c), draw(c.n, c.h, c.w, c.c)


def reference(c, x, w, dy):
    """float64 on the CPU: y, dx, dw in the layouts of make_data"""
    pad = geom(c)[0]
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().permute(2, 0, 1).unsqueeze(1).requires_grad_(True)      # [c, 1, 3, 3]
    y = F.conv2d(xr, wr, None, 1, pad, c.dil, groups=c.c)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous(),
            wr.grad.squeeze(1).permute(1, 2, 0).contiguous())


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


def run_all(hip_lib, lib, c, x, w, dy, base):
    """forward, dgrad (overwrite), dgrad (accumulate onto base), wgrad: the four active slices"""
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    pad, ho, wo, c_ld, ldx, ldy = geom(c)
    d = make_desc(lib, c)
    db, st = ctypes.byref(d), current_stream_ptr()
    xg, wg = padded(x, ldx, NAN), padded(w.view(3, 3, 1, c.c), c_ld, NAN)
    dyg = padded(dy, ldy, NAN, c.y_c0)
    off = 4 * c.y_c0                                                        # bytes: the slice's base
    y = torch.full((c.n, ho, wo, ldy), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_dwconv2d_forward(db, xg.data_ptr(), wg.data_ptr(), None, y.data_ptr() + off, st), "fwd")
    dx = torch.full((c.n, c.h, c.w, ldx), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_dwconv2d_dgrad(db, dyg.data_ptr() + off, wg.data_ptr(), dx.data_ptr(), 0, st), "dgrad")
    dxa = padded(base, ldx, SENTINEL)
    lib.check(hip_lib.gs_dwconv2d_dgrad(db, dyg.data_ptr() + off, wg.data_ptr(), dxa.data_ptr(), 1, st), "dgrad+")
    need = hip_lib.gs_dwconv2d_workspace_bytes(db)
    assert need > 0
    ws = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
    ws[:need] = 0xFF
    ws[need:] = GUARD_BYTE
    dw = torch.full((3, 3, 1, c_ld), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_dwconv2d_wgrad(db, xg.data_ptr(), dyg.data_ptr() + off, dw.data_ptr(), ws.data_ptr(),
                                        need, st), "wgrad")
    got = (active(y, c.y_c0, c.c, "y"), active(dx, 0, c.c, "dx"), active(dxa, 0, c.c, "dx+"),
           active(dw, 0, c.c, "dw").view(3, 3, c.c))
    assert bool((ws[need:] == GUARD_BYTE).all()), "the partials overran the workspace"
    return got


@pytest.mark.parametrize("case", CASES, ids=DCase.id)
def test_dwconv_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    c = case
    # (a) exact
    x, w, dy, base = make_data(c, True, 11)
    y_r, dx_r, dw_r = reference(c, x, w, dy)
    want = (y_r, dx_r, dx_r + base.double(), dw_r)
    assert max(float(t.abs().max()) for t in want) < 2 ** 24
    print("%s: exact leg, max |y| %g |dx| %g |dw| %g" % (c.id(), float(y_r.abs().max()), float(dx_r.abs().max()),
                                                          float(dw_r.abs().max())))
    for name, got, ref in zip(("y", "dx", "dx+", "dw"), run_all(hip_lib, lib, c, x, w, dy, base), want):
        assert torch.equal(got.double(), ref), "exact leg, %s: %d of %d elements differ, largest by %g" % (
            name, int((got.double() != ref).sum()), ref.numel(), float((got.double() - ref).abs().max()))
    # (b) random, twice
    x, w, dy, base = make_data(c, False, 12)
    y_r, dx_r, dw_r = reference(c, x, w, dy)
    want = (y_r, dx_r, dx_r + base.double(), dw_r)
    first = run_all(hip_lib, lib, c, x, w, dy, base)
    second = run_all(hip_lib, lib, c, x, w, dy, base)
    for name, a, b, ref in zip(("y", "dx", "dx+", "dw"), first, second, want):
        err = rel_err(a, ref)
        print("%s: random leg, %s rel_err %.3g" % (c.id(), name, err))
        assert err < TOL, name
        assert torch.equal(a, b), "%s: two runs of the same input differ" % name


def test_forward_bias_is_added_to_the_active_channels(hip_lib):
    """the optional bias of gs_dwconv2d_forward (a depthwise DynConv2d without a norm layer)"""
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    c = DCase(2, 5, 7, 20, dil=2, c_max=32, ldx=24)
    x, w, dy, _ = make_data(c, True, 13)
    bias = small_ints(torch.Generator().manual_seed(14), c.c)
    d = make_desc(lib, c)
    xg, wg, bg = padded(x, 24, NAN), padded(w.view(3, 3, 1, c.c), 32, NAN), padded(bias, 32, NAN)
    y = torch.full((c.n, c.h, c.w, c.c), SENTINEL, device=DEV)
    lib.check(hip_lib.gs_dwconv2d_forward(ctypes.byref(d), xg.data_ptr(), wg.data_ptr(), bg.data_ptr(),
                                          y.data_ptr(), current_stream_ptr()), "fwd")
    assert torch.equal(active(y, 0, c.c, "y").double(), reference(c, x, w, dy)[0] + bias.double())
