"""The ConvNeXt operators through the C-ABI (gs_dwconv2d_* with KH = KW = 7, gs_layernorm_*, gs_gelu_*,
gs_layer_scale_*; csrc/dwconv.hip, csrc/convnext_ops.hip), under the protocol of tests/test_dwconv_gpu.py:

  * outputs are pre-filled with a sentinel: everything outside the written slice -- pad columns of a wide
    pitch, the neighbours of a concat slice, parameter channels C .. C_max-1 -- must still hold it;
  * pad columns of the inputs beyond C, and parameter channels beyond C, hold NaN;
  * workspaces are exactly the queried size, hold NaN (0xFF), and sit in front of a 4 KiB guard;
  * every case runs twice and the two results are bit-identical (fixed reduction order, no atomics).

The depthwise 7x7 has an exact leg (nonzero integers in {+-1, +-2, +-3}: every partial sum is an integer
below 2^24, so fp32 is exact in any order and torch.equal against float64 holds) and a random leg at
TOL = 3e-5, that file's bound for fp32 operators.  One 3x3 case is compared bit for bit with the result
the library gave before the 7x7 kernels were added (tests/golden/dwconv3x3_parent.npz)."""
import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_convnext as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5
SENTINEL = 7.0
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
NAN = float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv3x3_parent.npz")


class DCase(NamedTuple):
    n: int
    h: int
    w: int
    c: int
    k: int = 7
    dil: int = 1
    pad: Optional[int] = None      # default: 'same'
    c_max: Optional[int] = None    # weight channels (C_ld)
    ldx: Optional[int] = None
    ldy: Optional[int] = None      # width of the buffer y / dy is a slice of
    y_c0: int = 0                  # first channel of that slice

    def id(self):
        s = "%dx%dx%dx%d-k%d-d%d" % (self.n, self.h, self.w, self.c, self.k, self.dil)
        if self.pad is not None:
            s += "-p%d" % self.pad
        if self.c_max:
            s += "-of%d" % self.c_max
        if self.ldx:
            s += "-ldx%d" % self.ldx
        if self.ldy:
            s += "-slice%dof%d" % (self.y_c0, self.ldy)
        return s


CASES7 = [
    DCase(2, 9, 11, 8),                                        # every border; interior below two kernels
    DCase(1, 5, 6, 4),                                         # image smaller than the kernel
    DCase(1, 1, 1, 8),                                         # only the centre tap is live
    DCase(2, 13, 17, 8, c_max=12, ldx=16, ldy=24, y_c0=8),     # 442 pixels: two reduction runs, ragged tail
    DCase(1, 8, 8, 4, dil=2, pad=6),
]
CASE3 = DCase(1, 33, 17, 12, k=3, dil=2)                       # from the table of tests/test_dwconv_gpu.py


def geom(c):
    pad = c.dil * (c.k // 2) if c.pad is None else c.pad
    ho, wo = c.h + 2 * pad - (c.k - 1) * c.dil, c.w + 2 * pad - (c.k - 1) * c.dil
    return pad, ho, wo, c.c_max or c.c, c.ldx or c.c, c.ldy or c.c


def small_ints(gen, *shape):
    return (torch.randint(1, 4, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def make_dw_data(c, exact, seed):
    """x [n,h,w,c], w [k,k,c], dy [n,ho,wo,c], base (the dx an accumulating dgrad adds to)"""
    _, ho, wo, _, _, _ = geom(c)
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda *s: small_ints(gen, *s)) if exact else (lambda *s: torch.randn(*s, generator=gen))
    return draw(c.n, c.h, c.w, c.c), draw(c.k, c.k, c.c), draw(c.n, ho, wo, c.c), draw(c.n, c.h, c.w, c.c)


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


class Workspace:
    """exactly ``need`` bytes of NaN in front of a guard"""

    def __init__(self, need):
        assert need > 0
        self.need = need
        self.buf = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
        self.buf[:need] = 0xFF
        self.buf[need:] = GUARD_BYTE

    def ptr(self):
        return self.buf.data_ptr()

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.need:] == GUARD_BYTE).all()), "the partials overran the workspace"


def stream():
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    return current_stream_ptr()


def run_dw(L, lib, c, x, w, dy, base):
    """forward, dgrad (overwrite), dgrad (accumulate onto base), wgrad through the library handle L"""
    pad, ho, wo, c_ld, ldx, ldy = geom(c)
    d = lib.dwconv_desc(c.n, c.h, c.w, c.c, pad, c.dil, c_ld=c_ld, ldx=ldx, ldy=ldy, k=c.k)
    db, st = ctypes.byref(d), stream()
    xg, wg = padded(x, ldx, NAN), padded(w.view(c.k, c.k, 1, c.c), c_ld, NAN)
    dyg = padded(dy, ldy, NAN, c.y_c0)
    off = 4 * c.y_c0
    y = torch.full((c.n, ho, wo, ldy), SENTINEL, device=DEV)
    lib.check(L.gs_dwconv2d_forward(db, xg.data_ptr(), wg.data_ptr(), None, y.data_ptr() + off, st), "fwd")
    dx = torch.full((c.n, c.h, c.w, ldx), SENTINEL, device=DEV)
    lib.check(L.gs_dwconv2d_dgrad(db, dyg.data_ptr() + off, wg.data_ptr(), dx.data_ptr(), 0, st), "dgrad")
    dxa = padded(base, ldx, SENTINEL)
    lib.check(L.gs_dwconv2d_dgrad(db, dyg.data_ptr() + off, wg.data_ptr(), dxa.data_ptr(), 1, st), "dgrad+")
    ws = Workspace(L.gs_dwconv2d_workspace_bytes(db))
    dw = torch.full((c.k, c.k, 1, c_ld), SENTINEL, device=DEV)
    lib.check(L.gs_dwconv2d_wgrad(db, xg.data_ptr(), dyg.data_ptr() + off, dw.data_ptr(), ws.ptr(), ws.need, st),
              "wgrad")
    got = (active(y, c.y_c0, c.c, "y"), active(dx, 0, c.c, "dx"), active(dxa, 0, c.c, "dx+"),
           active(dw, 0, c.c, "dw").view(c.k, c.k, c.c))
    ws.check()
    return got


def golden_3x3_inputs():
    return make_dw_data(CASE3, False, 21)


@pytest.mark.parametrize("case", CASES7, ids=DCase.id)
def test_dwconv7_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    c = case
    pad = geom(c)[0]
    # (a) exact
    x, w, dy, base = make_dw_data(c, True, 11)
    y_r, dx_r, dw_r = U.dwconv_ref(x, w, dy, pad, c.dil)
    want = (y_r, dx_r, dx_r + base.double(), dw_r)
    assert max(float(t.abs().max()) for t in want) < 2 ** 24
    for name, got, ref in zip(("y", "dx", "dx+", "dw"), run_dw(hip_lib, lib, c, x, w, dy, base), want):
        assert torch.equal(got.double(), ref), "exact leg, %s: %d of %d elements differ, largest by %g" % (
            name, int((got.double() != ref).sum()), ref.numel(), float((got.double() - ref).abs().max()))
    # (b) random, twice
    x, w, dy, base = make_dw_data(c, False, 12)
    y_r, dx_r, dw_r = U.dwconv_ref(x, w, dy, pad, c.dil)
    want = (y_r, dx_r, dx_r + base.double(), dw_r)
    first = run_dw(hip_lib, lib, c, x, w, dy, base)
    second = run_dw(hip_lib, lib, c, x, w, dy, base)
    for name, a, b, ref in zip(("y", "dx", "dx+", "dw"), first, second, want):
        err = rel_err(a, ref)
        print("%s: random leg, %s rel_err %.3g" % (c.id(), name, err))
        assert err < TOL, name
        assert torch.equal(a, b), "%s: two runs of the same input differ" % name


def test_dwconv3_is_bit_identical_to_the_library_before_the_7x7_kernels(hip_lib):
    """the stored outputs came from the previous library on an MI355X, for the inputs stored beside them"""
    from gaia_seg_amd.hip import lib
    g = np.load(GOLDEN)
    x, w, dy, base = golden_3x3_inputs()
    for name, t in zip(("x", "w", "dy", "base"), (x, w, dy, base)):
        assert np.array_equal(g[name], t.numpy()), "the generator no longer reproduces the stored %s" % name
    for name, got in zip(("y", "dx", "dxa", "dw"), run_dw(hip_lib, lib, CASE3, x, w, dy, base)):
        assert np.array_equal(g[name], got.numpy()), "3x3 %s changed" % name


# ---- LayerNorm -------------------------------------------------------------------------------------
LN_SHAPES = [(105, 4), (105, 8), (37, 96), (19, 260), (7, 1024)]
EPS = 1e-6


def run_ln(L, lib, x, weight, bias, dy, base):
    """forward, backward (overwrite), backward (accumulate onto base): y, mean, rstd, dx, dx+, dw, db"""
    rows, c = x.shape
    ld, c_max = c + 8, c + 4
    d = lib.layernorm_desc(rows, c, EPS, ldx=ld, ldy=ld)
    db, st = ctypes.byref(d), stream()
    xg, dyg = padded(x, ld, NAN), padded(dy, ld, NAN)
    wg, bg = padded(weight, c_max, NAN), padded(bias, c_max, NAN)
    y = torch.full((rows, ld), SENTINEL, device=DEV)
    stats = torch.full((2, rows + 16), SENTINEL, device=DEV)
    mean, rstd = stats[0], stats[1]
    lib.check(L.gs_layernorm_forward(db, xg.data_ptr(), wg.data_ptr(), bg.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), st), "ln fwd")
    outs = {}
    for key, acc in (("dx", 0), ("dx+", 1)):
        dx = padded(base, ld, SENTINEL) if acc else torch.full((rows, ld), SENTINEL, device=DEV)
        dwt, dbs = torch.full((c_max,), SENTINEL, device=DEV), torch.full((c_max,), SENTINEL, device=DEV)
        ws = Workspace(L.gs_layernorm_workspace_bytes(db))
        lib.check(L.gs_layernorm_backward(db, xg.data_ptr(), dyg.data_ptr(), wg.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), dx.data_ptr(), dwt.data_ptr(), dbs.data_ptr(), acc,
                                          ws.ptr(), ws.need, st), "ln bwd")
        outs[key] = active(dx, 0, c, key)
        outs["dw" + key[2:]], outs["db" + key[2:]] = active(dwt, 0, c, "dweight"), active(dbs, 0, c, "dbias")
        ws.check()
    assert torch.equal(outs["dw"], outs["dw+"]) and torch.equal(outs["db"], outs["db+"])
    return (active(y, 0, c, "y"), active(mean, 0, rows, "mean"), active(rstd, 0, rows, "rstd"), outs["dx"],
            outs["dx+"], outs["dw"], outs["db"])


@pytest.mark.parametrize("rows,c", LN_SHAPES, ids=lambda v: str(v))
def test_layernorm_kernels(hip_lib, rows, c):
    from gaia_seg_amd.hip import lib
    gen = torch.Generator().manual_seed(31 + c)
    x, dy, base = (torch.randn(rows, c, generator=gen) for _ in range(3))
    x[0] = 2.5                                                   # a constant row: zero variance
    weight, bias = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    ref = U.layernorm_ref(x, weight, bias, dy, EPS)
    want = ref[:4] + (ref[3] + base.double(),) + ref[4:]
    first = run_ln(hip_lib, lib, x, weight, bias, dy, base)
    second = run_ln(hip_lib, lib, x, weight, bias, dy, base)
    assert torch.equal(first[0][0], bias), "a constant row must give exactly the bias"
    for name, a, b, r in zip(("y", "mean", "rstd", "dx", "dx+", "dweight", "dbias"), first, second, want):
        err = rel_err(a, r)
        print("ln %dx%d: %s rel_err %.3g" % (rows, c, name, err))
        assert err < TOL, name
        assert torch.equal(a, b), "%s: two runs of the same input differ" % name


@pytest.mark.parametrize("rows,c", LN_SHAPES, ids=lambda v: str(v))
def test_layernorm_forward_with_a_large_common_offset(hip_lib, rows, c):
    """every row sits at 1e3: the statistics must not lose the row's spread in the offset"""
    from gaia_seg_amd.hip import lib
    gen = torch.Generator().manual_seed(41 + c)
    x = torch.randn(rows, c, generator=gen) + 1e3
    dy, base = torch.randn(rows, c, generator=gen), torch.zeros(rows, c)
    weight, bias = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    y_r = U.layernorm_ref(x, weight, bias, dy, EPS)[0]
    y = run_ln(hip_lib, lib, x, weight, bias, dy, base)[0]
    err = rel_err(y, y_r)
    print("ln %dx%d at offset 1e3: y rel_err %.3g (torch CPU fp32 F.layer_norm: %.3g)" % (
        rows, c, err, rel_err(F.layer_norm(x, (c,), weight, bias, EPS), y_r)))
    assert err < TOL


def test_layernorm_op_on_a_frozen_channel_slice(hip_lib):
    """ops.layernorm (the tape op) on the leading 8 channels of a 16-wide buffer that needs no gradient:
    the kernel still produces dx and addresses it with the input's pitch, so its scratch must have that
    pitch (ops._grad_target); the parameter gradients against the fp32 formula on the CPU."""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    gen = torch.Generator().manual_seed(53)
    xc, dy = torch.randn(1, 2, 3, 8, generator=gen), torch.randn(1, 2, 3, 8, generator=gen)
    wc, bc = torch.randn(8, generator=gen), torch.randn(8, generator=gen)
    buf = padded(xc, 16, SENTINEL)
    x = Act(buf[..., :8], requires_grad=False)
    weight, bias = torch.nn.Parameter(wc.to(DEV)), torch.nn.Parameter(bc.to(DEV))
    tape = Tape()
    out = ops.layernorm(tape, x, weight, bias, EPS)
    out.new_grad().copy_(dy.to(DEV))
    tape.backward()
    torch.cuda.synchronize()
    wr, br = wc.clone().requires_grad_(True), bc.clone().requires_grad_(True)
    y_r = F.layer_norm(xc, (8,), wr, br, EPS)
    y_r.backward(dy)
    assert x.g is None
    assert torch.equal(active(buf, 0, 8, "x"), xc)               # the input buffer is as it was
    for name, a, r in (("y", out.t, y_r), ("dweight", weight.grad, wr.grad), ("dbias", bias.grad, br.grad)):
        err = rel_err(a, r)
        print("ln op on a frozen slice: %s rel_err %.3g" % (name, err))
        assert err < TOL, name


# ---- GELU and layer scale ----------------------------------------------------------------------------
PW_SHAPES = [(105, 8), (19, 260)]


@pytest.mark.parametrize("rows,c", PW_SHAPES, ids=lambda v: str(v))
def test_gelu_kernels(hip_lib, rows, c):
    from gaia_seg_amd.hip import lib
    gen = torch.Generator().manual_seed(51 + c)
    x = torch.linspace(-6, 6, rows * c)[torch.randperm(rows * c, generator=gen)].view(rows, c).contiguous()
    x[3, 1] = 0.0
    x[0, 0], x[0, 1] = -6.0, 6.0
    dy = torch.randn(rows, c, generator=gen)
    y_r, dx_r = U.gelu_ref(x, dy)
    ldx, ldy, lddx = c + 8, c + 4, c + 12
    res = []
    for _ in range(2):
        xg, dyg = padded(x, ldx, NAN), padded(dy, ldy, NAN)
        y = torch.full((rows, ldy), SENTINEL, device=DEV)
        dx = torch.full((rows, lddx), SENTINEL, device=DEV)
        lib.check(hip_lib.gs_gelu_forward(xg.data_ptr(), y.data_ptr(), rows, c, ldx, ldy, stream()), "gelu fwd")
        lib.check(hip_lib.gs_gelu_backward(xg.data_ptr(), dyg.data_ptr(), dx.data_ptr(), rows, c, ldx, ldy, lddx,
                                           stream()), "gelu bwd")
        res.append((active(y, 0, c, "y"), active(dx, 0, c, "dx")))
    for name, a, b, r in zip(("y", "dx"), res[0], res[1], (y_r, dx_r)):
        err = rel_err(a, r)
        print("gelu %dx%d: %s rel_err %.3g" % (rows, c, name, err))
        assert err < TOL, name
        assert torch.equal(a, b)
    assert float(res[0][0][3, 1]) == 0.0


@pytest.mark.parametrize("rows,c", PW_SHAPES, ids=lambda v: str(v))
def test_layer_scale_kernels(hip_lib, rows, c):
    from gaia_seg_amd.hip import lib
    gen = torch.Generator().manual_seed(61 + c)
    ident, z, dout = (torch.randn(rows, c, generator=gen) for _ in range(3))
    gamma = torch.randn(c, generator=gen)
    out_r, dz_r, dg_r = U.layer_scale_ref(ident, z, gamma, dout)
    ldi, ldz, ldo, c_max = c + 4, c + 8, c + 12, c + 4
    res = []
    for _ in range(2):
        ig, zg, dog, gg = padded(ident, ldi, NAN), padded(z, ldz, NAN), padded(dout, ldo, NAN), padded(gamma, c_max, NAN)
        out = torch.full((rows, ldo), SENTINEL, device=DEV)
        dz = torch.full((rows, ldz), SENTINEL, device=DEV)
        dg = torch.full((c_max,), SENTINEL, device=DEV)
        lib.check(hip_lib.gs_layer_scale_add_forward(ig.data_ptr(), zg.data_ptr(), gg.data_ptr(), out.data_ptr(), rows,
                                                     c, ldi, ldz, ldo, stream()), "ls fwd")
        ws = Workspace(hip_lib.gs_layer_scale_workspace_bytes(rows, c))
        lib.check(hip_lib.gs_layer_scale_backward(dog.data_ptr(), zg.data_ptr(), gg.data_ptr(), dz.data_ptr(),
                                                  dg.data_ptr(), rows, c, ldo, ldz, ldz, ws.ptr(), ws.need, stream()),
                  "ls bwd")
        res.append((active(out, 0, c, "out"), active(dz, 0, c, "dz"), active(dg, 0, c, "dgamma")))
        ws.check()
    for name, a, b, r in zip(("out", "dz", "dgamma"), res[0], res[1], (out_r, dz_r, dg_r)):
        err = rel_err(a, r)
        print("layer scale %dx%d: %s rel_err %.3g" % (rows, c, name, err))
        assert err < TOL, name
        assert torch.equal(a, b)
