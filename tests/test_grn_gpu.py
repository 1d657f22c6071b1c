"""GELU + GRN on the GPU: gs_gelu_grn_* through the C-ABI (csrc/grn.hip) and ops.gelu_grn through the tape,
against the float64 CPU reference of tests/util_convnextv2.py (torch's F.gelu, torch.linalg.vector_norm and
autograd), under the protocol of tests/test_convnext_ops_gpu.py:

  * outputs are pre-filled with a sentinel: pad columns of a wide pitch and parameter channels C .. C_max-1
    must still hold it;
  * pad columns of the inputs beyond C, and parameter channels beyond C, hold NaN;
  * workspaces are exactly the queried size, hold NaN (0xFF), and sit in front of a 4 KiB guard;
  * every case runs twice and the two results are bit-identical (fixed reduction order, no atomics).

Bound: conftest.rel_err < 3e-5, that file's bound for fp32 operators (fp32 torch on the CPU sits at
1e-7 .. 5e-7 for these cases in y, dx, dweight and dbias)."""
import ctypes

import pytest
import torch

from conftest import rel_err
import util_convnextv2 as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5
EPS = 1e-6
SENTINEL = 7.0
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
NAN = float("nan")
NAMES = ("y", "G", "dx", "dweight", "dbias")

# (N, H, W, C, pitch)
CASES = [
    (2, 5, 7, 8, 8),           # less than one run, odd P
    (3, 24, 24, 96, 96),       # P = 576: runs of 256 cut over all rows would straddle the samples
    (2, 1, 1, 64, 64),         # P = 1, stage 4 of a tiny input
    (2, 16, 16, 136, 160),     # pitch above C, the last group of 16 channel quads partly filled
    (1, 33, 31, 260, 260),
]


def padded(t, ld, fill):
    """t [..., c] at the front of a [..., ld] buffer filled with ``fill``"""
    buf = torch.full(t.shape[:-1] + (ld,), fill)
    buf[..., :t.shape[-1]] = t
    return buf.to(DEV)


def active(buf, c, what):
    """synchronise; everything beyond [..., :c] still holds the sentinel; the slice on the CPU"""
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[..., c:] == SENTINEL).all()), "%s: a store outside the active slice" % what
    got = out[..., :c].contiguous()
    assert bool(torch.isfinite(got).all()), "%s: not finite -- a pad column or an unwritten partial was read" % what
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


def run_grn(L, x, weight, bias, dy, pitch, c_max, inplace=False):
    """forward and backward through the library handle L: x, dy [N, P, C] -> (y, G, dx, dweight, dbias)"""
    from gaia_seg_amd.hip import lib
    n, p, c = x.shape
    d = lib.gelu_grn_desc(n, p, c, EPS, ldx=pitch, ldy=pitch, lddy=pitch, lddx=pitch)
    db, st = ctypes.byref(d), stream()
    xg = padded(x, pitch, NAN)
    wg, bg = padded(weight, c_max, NAN), padded(bias, c_max, NAN)
    y = torch.full((n, p, pitch), SENTINEL, device=DEV)
    G = torch.full((n * c + 16,), SENTINEL, device=DEV)
    need = L.gs_gelu_grn_workspace_bytes(db)
    ws = Workspace(need)
    lib.check(L.gs_gelu_grn_forward(db, xg.data_ptr(), wg.data_ptr(), bg.data_ptr(), y.data_ptr(), G.data_ptr(),
                                    ws.ptr(), ws.need, st), "gelu_grn fwd")
    ws.check()
    if inplace:          # dx lands in dy's own buffer (its pad columns hold the sentinel, for active())
        dyg = dx = padded(dy, pitch, SENTINEL)
    else:
        dyg, dx = padded(dy, pitch, NAN), torch.full((n, p, pitch), SENTINEL, device=DEV)
    dwt, dbs = torch.full((c_max,), SENTINEL, device=DEV), torch.full((c_max,), SENTINEL, device=DEV)
    ws = Workspace(need)
    lib.check(L.gs_gelu_grn_backward(db, xg.data_ptr(), dyg.data_ptr(), wg.data_ptr(), G.data_ptr(), dx.data_ptr(),
                                     dwt.data_ptr(), dbs.data_ptr(), ws.ptr(), ws.need, st), "gelu_grn bwd")
    ws.check()
    return (active(y, c, "y"), active(G, n * c, "G").view(n, c), active(dx, c, "dx"), active(dwt, c, "dweight"),
            active(dbs, c, "dbias"))


def make_data(n, p, c, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, p, c, generator=gen) * 1.5
    dy = torch.randn(n, p, c, generator=gen)
    weight, bias = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    return x, weight, bias, dy


def compare(tag, first, second, want):
    for name, a, b, r in zip(NAMES, first, second, want):
        err = rel_err(a, r)
        print("%s: %s rel_err %.3g" % (tag, name, err))
        assert err < TOL, name
        assert torch.equal(a, b), "%s: two runs of the same input differ" % name


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_gelu_grn_kernels(hip_lib, case):
    n, h, w, c, pitch = case
    x, weight, bias, dy = make_data(n, h * w, c, 71 + c)
    want = U.gelu_grn_ref(x, weight, bias, dy, EPS)
    c_max = c if pitch == c else c + 4
    first = run_grn(hip_lib, x, weight, bias, dy, pitch, c_max)
    second = run_grn(hip_lib, x, weight, bias, dy, pitch, c_max)
    compare("grn %s" % (case,), first, second, want)


def test_a_zero_channel_and_a_zero_sample_stay_finite(hip_lib):
    """G == 0: the gradient through the norm is zero there (torch's convention for the 2-norm); a whole zero
    sample has mean G = 0 and Nx = 0 / eps = 0"""
    n, p, c = 3, 300, 24
    x, weight, bias, dy = make_data(n, p, c, 5)
    x[..., 3] = 0
    x[1] = 0
    want = U.gelu_grn_ref(x, weight, bias, dy, EPS)
    assert all(bool(torch.isfinite(t).all()) for t in want)
    first = run_grn(hip_lib, x, weight, bias, dy, 32, 28)
    second = run_grn(hip_lib, x, weight, bias, dy, 32, 28)
    compare("grn zeros", first, second, want)
    assert float(first[1][1].abs().max()) == 0 and float(first[1][:, 3].abs().max()) == 0
    assert torch.equal(first[0][1], bias.expand(p, c))              # y of the zero sample is exactly the bias
    assert float(first[2][1].abs().max()) > 0                       # dx = dy * gelu'(0) there, not zero


def test_a_leading_slice_of_wider_parameters_equals_the_standalone_width_bit_for_bit(hip_lib):
    """weight / bias are [64] with 24 active channels: entries 24.. of dweight / dbias keep the sentinel (run_grn
    asserts it), and the mean of G runs over the 24 active channels only -- slice == standalone"""
    n, p, c = 2, 270, 24
    x, weight, bias, dy = make_data(n, p, c, 6)
    want = U.gelu_grn_ref(x, weight, bias, dy, EPS)
    sliced = run_grn(hip_lib, x, weight, bias, dy, 4 * 64, 64)
    alone = run_grn(hip_lib, x, weight, bias, dy, c, c)
    compare("grn 24 of 64", sliced, alone, want)


def test_dx_written_into_dys_buffer_equals_the_out_of_place_result(hip_lib):
    n, p, c = 2, 520, 40
    x, weight, bias, dy = make_data(n, p, c, 7)
    want = U.gelu_grn_ref(x, weight, bias, dy, EPS)
    out_of_place = run_grn(hip_lib, x, weight, bias, dy, 48, 44)
    in_place = run_grn(hip_lib, x, weight, bias, dy, 48, 44, inplace=True)
    compare("grn in place", out_of_place, in_place, want)


# ---- the tape op and the brick --------------------------------------------------------------------------
def test_ops_gelu_grn_through_the_brick_on_an_active_slice(hip_lib):
    """DynamicGRN(64) on a 24-channel activation: ops.gelu_grn with the width of the incoming activation; the
    parameter gradients land in the leading slice and stay zero beyond it"""
    from gaia_seg_amd.core.bricks import DynamicGRN
    n, h, w, c, c_max = 2, 9, 30, 24, 64
    x, weight, bias, dy = make_data(n, h * w, c, 8)
    want = U.gelu_grn_ref(x, weight, bias, dy, EPS)
    gen = torch.Generator().manual_seed(1)
    m = DynamicGRN(c_max)
    assert tuple(m.weight.shape) == (1, 1, 1, c_max) and float(m.weight.abs().max()) == 0
    with torch.no_grad():
        m.weight.copy_(torch.randn(1, 1, 1, c_max, generator=gen))
        m.bias.copy_(torch.randn(1, 1, 1, c_max, generator=gen))
        m.weight[..., :c] = weight
        m.bias[..., :c] = bias
    m = m.to(DEV)
    res = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xg = x.view(n, h, w, c).to(DEV).requires_grad_(True)
        y = m(xg)
        assert tuple(y.shape) == (n, h, w, c)
        y.backward(dy.view(n, h, w, c).to(DEV))
        torch.cuda.synchronize()
        gw, gb = m.weight.grad.cpu(), m.bias.grad.cpu()
        assert tuple(gw.shape) == (1, 1, 1, c_max)
        assert float(gw[..., c:].abs().max()) == 0 and float(gb[..., c:].abs().max()) == 0
        res.append((y.detach().cpu().view(n, h * w, c), want[1].float(), xg.grad.cpu().view(n, h * w, c),
                    gw[0, 0, 0, :c], gb[0, 0, 0, :c]))
    compare("ops.gelu_grn", res[0], res[1], want)
    # deploy mode cuts the parameters to the active slice, and the result does not move
    m.deploy()
    with torch.no_grad():
        y = m(x.view(n, h, w, c).to(DEV))
    assert tuple(m.weight.shape) == (1, 1, 1, c) and tuple(m.bias.shape) == (1, 1, 1, c) and m.dim == c
    assert torch.equal(y.cpu().view(n, h * w, c), res[0][0])


def test_ops_gelu_grn_refusals(hip_lib):
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import tape_function
    w = torch.zeros(1, 1, 1, 8, device=DEV, requires_grad=True)
    b = torch.zeros(1, 1, 1, 8, device=DEV, requires_grad=True)

    def run(c, fn):
        x = torch.randn(1, c, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        return tape_function(lambda tape, acts: fn(tape, acts[0]), [x], True)

    with pytest.raises(ValueError, match="at most 8"):
        run(12, lambda tape, a: [ops.gelu_grn(tape, a, w, b)])
    with pytest.raises(ValueError, match="per-channel"):
        run(8, lambda tape, a: [ops.gelu_grn(tape, a, w, b[0, 0, 0])])
    # a second consumer of the pre-activation: its gradient would be overwritten, so the backward refuses
    outs = run(8, lambda tape, a: [ops.gelu_grn(tape, a, w, b), ops.gelu(tape, a)])
    with pytest.raises(RuntimeError, match="more than one consumer"):
        torch.autograd.backward(list(outs), [torch.ones_like(o) for o in outs])
