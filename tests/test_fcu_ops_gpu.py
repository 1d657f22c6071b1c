"""ElasticConvformer's coupling kernels through the C-ABI (gs_fcu_down_*, gs_fcu_up_add_*, gs_fcu_tokens_*;
csrc/fcu.hip) against float64, under the protocol of tests/test_convnext_ops_gpu.py:

  * outputs are pre-filled with a sentinel: everything outside the written slice -- pad columns of a wide
    pitch, parameter channels D .. D_max-1 -- must still hold it;
  * pad columns of the inputs beyond the width, and parameter channels beyond it, hold NaN;
  * workspaces are exactly the queried size, hold NaN (0xFF), and sit in front of a 4 KiB guard;
  * every case runs twice and the two results are bit-identical (fixed reduction order, no atomics).

Bound: rel_err against float64 at TOL = 3e-5, the project's bound for fp32 operators."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_convformer as U
from test_convnext_ops_gpu import DEV, NAN, SENTINEL, TOL, Workspace, active, padded, stream

pytestmark = pytest.mark.gpu
EPS = 1e-5

# (B, T, D)
DOWN_CASES = [(1, 1, 4),        # one token, one quad
              (2, 6, 72),       # a quad count that is no power of two
              (2, 6, 576),      # more quads than a wave has lanes
              (2, 135, 64)]     # 270 rows: crosses a 256-row run of the partials, and an image boundary off a run


def down_ref(z, x_t, weight, bias, dout):
    """float64 -> (out, mean, rstd, dz, dx_t, dweight, dbias)"""
    zr, xr, wr, br = (t.double().requires_grad_(True) for t in (z, x_t, weight, bias))
    out = U.fcu_down_ref(zr, xr, wr, br, EPS)
    out.backward(dout.double())
    mean = zr.detach().mean(-1)
    rstd = (zr.detach().var(-1, unbiased=False) + EPS).rsqrt()
    return out.detach(), mean, rstd, zr.grad, xr.grad, wr.grad, br.grad


def run_down(L, lib, z, x_t, weight, bias, dout, base, pitched):
    """forward, backward (overwrite), backward (accumulate onto base), all as rows x D:
    out, mean, rstd, dz, dx_t, dx_t+, dweight, dbias"""
    b, t, dch = z.shape
    pad = (8, 4, 12, 16, 20) if pitched else (0,) * 5
    ldz, ldxt, ldo, lddz, lddxt = (dch + p for p in pad)
    d_max = dch + 4
    d = lib.fcu_down_desc(b, t, dch, EPS, ldz=ldz, ldxt=ldxt, ldo=ldo, lddz=lddz, lddxt=lddxt)
    db, st = ctypes.byref(d), stream()
    zg, xg = padded(z.reshape(b * t, dch), ldz, NAN), padded(x_t.reshape(b * (t + 1), dch), ldxt, NAN)
    dog = padded(dout.reshape(b * (t + 1), dch), ldo, NAN)
    wg, bg = padded(weight, d_max, NAN), padded(bias, d_max, NAN)
    out = torch.full((b * (t + 1), ldo), SENTINEL, device=DEV)
    stats = torch.full((2, b * t + 16), SENTINEL, device=DEV)
    mean, rstd = stats[0], stats[1]
    lib.check(L.gs_fcu_down_forward(db, zg.data_ptr(), xg.data_ptr(), wg.data_ptr(), bg.data_ptr(), out.data_ptr(),
                                    mean.data_ptr(), rstd.data_ptr(), st), "fcu_down fwd")
    res = {}
    for key, acc in (("", 0), ("+", 1)):
        dxt = (padded(base.reshape(b * (t + 1), dch), lddxt, SENTINEL) if acc
               else torch.full((b * (t + 1), lddxt), SENTINEL, device=DEV))
        dz = torch.full((b * t, lddz), SENTINEL, device=DEV)
        dwt, dbs = torch.full((d_max,), SENTINEL, device=DEV), torch.full((d_max,), SENTINEL, device=DEV)
        ws = Workspace(L.gs_fcu_down_workspace_bytes(db))
        lib.check(L.gs_fcu_down_backward(db, zg.data_ptr(), dog.data_ptr(), wg.data_ptr(), bg.data_ptr(),
                                         mean.data_ptr(), rstd.data_ptr(), dz.data_ptr(), dxt.data_ptr(),
                                         dwt.data_ptr(), dbs.data_ptr(), acc, ws.ptr(), ws.need, st), "fcu_down bwd")
        res["dxt" + key], res["dz" + key] = active(dxt, 0, dch, "dx_t" + key), active(dz, 0, dch, "dz")
        res["dw" + key], res["db" + key] = active(dwt, 0, dch, "dweight"), active(dbs, 0, dch, "dbias")
        ws.check()
    for k in ("dz", "dw", "db"):
        assert torch.equal(res[k], res[k + "+"]), "%s depends on the accumulate flag of dx_t" % k
    return (active(out, 0, dch, "out"), active(mean, 0, b * t, "mean"), active(rstd, 0, b * t, "rstd"), res["dz"],
            res["dxt"], res["dxt+"], res["dw"], res["db"])


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("case", DOWN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fcu_down_kernels(hip_lib, case, pitched):
    from gaia_seg_amd.hip import lib
    b, t, dch = case
    gen = torch.Generator().manual_seed(71 + dch + t)
    z = torch.randn(b, t, dch, generator=gen)
    x_t, dout, base = (torch.randn(b, t + 1, dch, generator=gen) for _ in range(3))
    weight, bias = torch.rand(dch, generator=gen) + 0.5, torch.randn(dch, generator=gen) * 0.5
    ref = down_ref(z, x_t, weight, bias, dout)
    want = ref[:5] + (ref[4] + base.double(),) + ref[5:]
    first = run_down(hip_lib, lib, z, x_t, weight, bias, dout, base, pitched)
    second = run_down(hip_lib, lib, z, x_t, weight, bias, dout, base, pitched)
    names = ("out", "mean", "rstd", "dz", "dx_t", "dx_t+", "dweight", "dbias")
    for name, a, bb, r in zip(names, first, second, want):
        err = rel_err(a, r.reshape(a.shape))
        print("fcu_down %s%s: %s rel_err %.3g" % (case, " pitched" if pitched else "", name, err))
        assert err < TOL, name
        assert torch.equal(a, bb), "%s: two runs of the same input differ" % name
    # bit for bit: the cls rows of out are x_t + x_t; dx_t is dout on token rows and 2 dout on cls rows
    out, dxt = first[0].view(b, t + 1, dch), first[4].view(b, t + 1, dch)
    assert torch.equal(out[:, 0], x_t[:, 0] + x_t[:, 0])
    assert torch.equal(dxt[:, 1:], dout[:, 1:]) and torch.equal(dxt[:, 0], 2 * dout[:, 0])


# (B, H / s, W / s, C, s, pitched)
UP_CASES = [(1, 1, 1, 4, 4, False),      # a single coarse cell
            (2, 3, 5, 68, 2, True),      # odd coarse sizes, pitched
            (2, 3, 5, 8, 1, False),      # s = 1
            (2, 2, 3, 32, 4, False)]     # s = 4


def run_up(L, lib, x, r, dout, base, s, pitched):
    """out, dr, dr+ as NHWC tensors"""
    b, h, w, c = x.shape
    ldx, ldr, ldo, lddo, lddr = ((c + 4, c + 8, c + 12, c + 16, c + 20) if pitched else (c,) * 5)
    st = stream()
    xg, rg, dog = padded(x, ldx, NAN), padded(r, ldr, NAN), padded(dout, lddo, NAN)
    out = torch.full((b, h, w, ldo), SENTINEL, device=DEV)
    lib.check(L.gs_fcu_up_add_forward(xg.data_ptr(), rg.data_ptr(), out.data_ptr(), b, h, w, c, s, ldx, ldr, ldo, st),
              "fcu_up_add fwd")
    dr = torch.full(r.shape[:3] + (lddr,), SENTINEL, device=DEV)
    dra = padded(base, lddr, SENTINEL)
    for buf, acc in ((dr, 0), (dra, 1)):
        lib.check(L.gs_fcu_up_add_backward(dog.data_ptr(), buf.data_ptr(), b, h, w, c, s, lddo, lddr, acc, st),
                  "fcu_up_add bwd")
    return active(out, 0, c, "out"), active(dr, 0, c, "dr"), active(dra, 0, c, "dr+")


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "x".join(map(str, c[:5])))
def test_fcu_up_add_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    b, hc, wc, c, s, pitched = case
    gen = torch.Generator().manual_seed(81 + c + s)
    x, dout = (torch.randn(b, hc * s, wc * s, c, generator=gen) for _ in range(2))
    r, base = (torch.randn(b, hc, wc, c, generator=gen) for _ in range(2))
    nchw = lambda t: t.permute(0, 3, 1, 2)   # noqa: E731
    want_out = U.fcu_up_add_ref(nchw(x), nchw(r), s).permute(0, 2, 3, 1).contiguous()   # fp32 torch: one add
    rr = r.double().requires_grad_(True)
    U.fcu_up_add_ref(nchw(x.double()), nchw(rr), s).backward(nchw(dout.double()))
    first = run_up(hip_lib, lib, x, r, dout, base, s, pitched)
    second = run_up(hip_lib, lib, x, r, dout, base, s, pitched)
    assert torch.equal(first[0], want_out), "the forward is one fp32 add and must equal torch bit for bit"
    if s == 1:
        assert torch.equal(first[1], dout), "at s = 1 dr is dout"
    for name, a, bb, ref in zip(("out", "dr", "dr+"), first, second, (want_out, rr.grad, rr.grad + base.double())):
        err = rel_err(a, ref)
        print("fcu_up_add %s: %s rel_err %.3g" % (case[:5], name, err))
        assert err < TOL, name
        assert torch.equal(a, bb), "%s: two runs of the same input differ" % name


@pytest.mark.parametrize("case", [(1, 1, 4), (3, 6, 72)], ids=lambda c: "x".join(map(str, c)))
def test_fcu_tokens_kernels(hip_lib, case):
    from gaia_seg_amd.hip import lib
    b, t, dch = case
    gen = torch.Generator().manual_seed(91 + dch)
    patches, cls = torch.randn(b, t, dch, generator=gen), torch.randn(dch, generator=gen)
    dx = torch.randn(b, t + 1, dch, generator=gen)
    ldp, ldx, d_max = dch + 8, dch + 4, dch + 12
    res = []
    for _ in range(2):
        pg, cg = padded(patches.reshape(b * t, dch), ldp, NAN), padded(cls, d_max, NAN)
        dxg = padded(dx.reshape(b * (t + 1), dch), ldx, NAN)
        x = torch.full((b * (t + 1), ldx), SENTINEL, device=DEV)
        dp = torch.full((b * t, ldp), SENTINEL, device=DEV)
        dc = torch.full((d_max,), SENTINEL, device=DEV)
        lib.check(hip_lib.gs_fcu_tokens_forward(pg.data_ptr(), ldp, cg.data_ptr(), x.data_ptr(), ldx, b, t, dch,
                                                stream()), "fcu_tokens fwd")
        lib.check(hip_lib.gs_fcu_tokens_backward(dxg.data_ptr(), ldx, dp.data_ptr(), ldp, dc.data_ptr(), b, t, dch,
                                                 stream()), "fcu_tokens bwd")
        res.append((active(x, 0, dch, "x"), active(dp, 0, dch, "dpatches"), active(dc, 0, dch, "dcls")))
    x, dp, dc = res[0]
    assert torch.equal(x.view(b, t + 1, dch), torch.cat([cls.expand(b, 1, dch), patches], dim=1))
    assert torch.equal(dp.view(b, t, dch), dx[:, 1:])
    assert rel_err(dc, dx[:, 0].double().sum(0)) < TOL
    for a, bb in zip(res[0], res[1]):
        assert torch.equal(a, bb)
