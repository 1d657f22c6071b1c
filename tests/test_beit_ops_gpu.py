"""gs_attention_relpos_forward and gs_deconv2x2_forward through the C-ABI, under the protocol of
tests/test_attention_gpu.py: outputs pre-filled with a sentinel, NaN in every pad column and in the idle
head of the inputs, two runs that must agree bit for bit, float64 restatements (tests/util_beit.py) and the
bounds of the operators they extend -- TOL = 3e-5 in conftest.rel_err for O and lse (test_attention_gpu.py)
and for the deconvolution (test_hip_ops_gpu.py's bound for the gs_conv2d forward).

Table entries are N(0, 2^2): CONDITION, checked on the float64 restatement alone before anything runs on
the GPU -- the output with the table differs from the output without it by more than 100 x TOL, so a
kernel that ignored the bias, or read the wrong rows, could not pass."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_beit as B
import util_vit as U
from util_attention_gpu import NAN, RELPOS_CASES, SENTINEL, active, make_table, run_relpos, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5

@pytest.mark.parametrize("case", RELPOS_CASES, ids=[c[0] for c in RELPOS_CASES])
def test_relpos_attention_forward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    name, b, wh, ww, heads, sliced, cls_only = case
    n = wh * ww + 1
    q, k, v = U.attention_inputs(b, n, heads, False, 7)[:3]
    table = make_table(wh, ww, heads, cls_only, 11)
    o_r, lse_r = B.relpos_attention(q.double(), k.double(), v.double(), heads, table.double(), wh, ww)
    o_plain, _ = B.relpos_attention(q.double(), k.double(), v.double(), heads, None, wh, ww)
    effect = rel_err(o_plain, o_r)
    print(name, "bias effect on O %.3g" % effect)
    assert effect > 100 * TOL, "the table does not change the float64 output enough to be seen"
    if not cls_only:     # a transposed window reads other rows: the restatement itself tells them apart
        o_swap, _ = B.relpos_attention(q.double(), k.double(), v.double(), heads, table.double(), ww, wh)
        assert rel_err(o_swap, o_r) > 100 * TOL
    first = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, table)
    second = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, table)
    errs = {nm: rel_err(g, r) for nm, g, r in zip(("O", "lse"), first, (o_r, lse_r))}
    print(name, {nm: "%.2e" % e for nm, e in errs.items()})
    for nm, a, bb in zip(("O", "lse"), first, second):
        assert torch.equal(a, bb), "%s differs between two runs" % nm
    for nm, e in errs.items():
        assert e < TOL, "%s: rel_err %.3g" % (nm, e)


@pytest.mark.parametrize("case", [RELPOS_CASES[0], RELPOS_CASES[3]], ids=["2x3", "11x12-sliced"])
def test_a_zero_table_gives_the_bits_of_the_bias_free_forward(hip_lib, case):
    from gaia_seg_amd.hip import lib
    _, b, wh, ww, heads, sliced, _ = case
    q, k, v = U.attention_inputs(b, wh * ww + 1, heads, False, 7)[:3]
    zero = torch.zeros((2 * wh - 1) * (2 * ww - 1) + 3, heads)
    o_b, lse_b = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, zero)
    o_p, lse_p = run_relpos(hip_lib, lib, b, wh, ww, heads, sliced, q, k, v, None)
    assert torch.equal(o_b, o_p), "O: a zero table changes bits"
    assert torch.equal(lse_b, lse_p), "lse: a zero table changes bits"


def test_relpos_refusals_leave_the_outputs_alone(hip_lib):
    from gaia_seg_amd.hip import lib
    L, st = hip_lib, stream()
    x = torch.zeros(1, 7, 64, device=DEV)
    o = torch.full((1, 7, 64), SENTINEL, device=DEV)
    lse = torch.full((7,), SENTINEL, device=DEV)
    t = torch.zeros(18, 1, device=DEV)
    p = x.data_ptr()
    d = lib.attention_desc(1, 7, 1, U.SCALE)
    args = (o.data_ptr(), lse.data_ptr(), st)
    assert L.gs_attention_relpos_forward(ctypes.byref(d), p, p, p, None, 1, 2, 3, *args) == -4
    assert L.gs_attention_relpos_forward(ctypes.byref(d), p, p, p, t.data_ptr(), 1, 3, 3, *args) == -1
    assert L.gs_attention_relpos_forward(ctypes.byref(d), p, p, p, t.data_ptr(), 0, 2, 3, *args) == -1
    assert L.gs_attention_relpos_forward(ctypes.byref(d), p + 4, p, p, t.data_ptr(), 1, 2, 3, *args) == -2
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all()) and bool((lse == SENTINEL).all()), "a refused call wrote to an output"


# ---- ConvTranspose2d(2, 2) -------------------------------------------------------------------------------
# (name, N, H, W, Cin, Cout, output pitch, bias?)
DECONV_CASES = [
    ("2x3x5-8to12", 2, 3, 5, 8, 12, 12, True),
    ("1x4x4-68to64-wide-pitch", 1, 4, 4, 68, 64, 72, True),
    ("2x3x5-8to12-no-bias", 2, 3, 5, 8, 12, 12, False),
]


def run_deconv(n, h, w, cin, cout, ldy, x, weight, bias):
    """ops.deconv2x2 on an input with NaN pad columns into a sentinel-filled output of pitch ldy"""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    ldx = cin + 4
    xb = torch.full((n, h, w, ldx), NAN)
    xb[..., :cin] = x.permute(0, 2, 3, 1)
    xb = xb.to(DEV)
    yb = torch.full((n, 2 * h, 2 * w, ldy), SENTINEL, device=DEV)
    ops.deconv2x2(Tape(enabled=False), Act(xb[..., :cin], False), weight, bias, out=Act(yb[..., :cout], False))
    return active(yb, 0, cout, "y").permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", DECONV_CASES, ids=[c[0] for c in DECONV_CASES])
def test_deconv2x2_forward(hip_lib, case):
    name, n, h, w, cin, cout, ldy, has_bias = case
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5
    bs = torch.randn(cout, generator=g) if has_bias else None
    want = F.conv_transpose2d(x.double(), wt.double(), bs.double() if has_bias else None, stride=2)
    weight = torch.nn.Parameter(wt.to(DEV), requires_grad=False)
    bias = torch.nn.Parameter(bs.to(DEV), requires_grad=False) if has_bias else None
    first = run_deconv(n, h, w, cin, cout, ldy, x, weight, bias)
    second = run_deconv(n, h, w, cin, cout, ldy, x, weight, bias)
    err = rel_err(first, want)
    print(name, "rel_err %.2e" % err)
    assert torch.equal(first, second), "two runs differ"
    assert err < TOL, err
    # the repacked copy follows an in-place change of the parameter
    with torch.no_grad():
        weight.mul_(-0.5)
        weight[0, 0, 1, 0] += 3.0
    want2 = F.conv_transpose2d(x.double(), weight.detach().cpu().double(), bs.double() if has_bias else None,
                               stride=2)
    assert rel_err(want2, want) > 100 * TOL
    err2 = rel_err(run_deconv(n, h, w, cin, cout, ldy, x, weight, bias), want2)
    assert err2 < TOL, "after an in-place change of the weight: %.3g" % err2


def test_deconv2x2_is_forward_only(hip_lib):
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    weight = torch.nn.Parameter(torch.zeros(8, 12, 2, 2, device=DEV))
    x = Act(torch.zeros(1, 2, 2, 8, device=DEV), True)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.deconv2x2(Tape(), x, weight, None)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.deconv2x2(Tape(enabled=False), Act(torch.zeros(1, 2, 2, 6, device=DEV), False),
                      torch.zeros(6, 12, 2, 2, device=DEV), None)
