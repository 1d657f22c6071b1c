"""The convolution weight gradient through the C-ABI (gs_conv2d_wgrad; csrc/igemm_wgrad.hip, the kernels
igemm_wgrad_fast_kernel / igemm_wgrad_kernel / splitk_reduce_kernel of csrc/igemm_core.h).

Every case runs on buffers that forgive nothing:

  * dw is the [KH][KW][Ci_max][Co_ld] weight pre-filled with a sentinel: everything outside the
    [:, :, :Ci, :Co] slice must still hold it afterwards;
  * the workspace is exactly gs_conv2d_workspace_bytes(d) bytes of NaN (0xFF) in front of a 4 KiB guard
    with a known byte pattern: a slab cell read before it was written turns the result NaN, a slab
    overrun breaks the guard;
  * x channels beyond Ci and dy columns beyond Co (wider pitches) hold NaN.

and with two kinds of data:

  (a) exact: x and dy are nonzero integers in {+-1, +-2, +-3}.  Every product and partial sum is an
      integer far below 2^24 (largest |dw| here: 2703, at 16384 pixels), so fp32 accumulation is exact
      in any order, under any split count and either form of the reduce: torch.equal against float64.
      One dropped, duplicated or misplaced pixel or tap moves an element by at least 1.
  (b) random: standard normal x and dy against the float64 reference within TOL = 3e-5 (the bound of
      the other fp32 MFMA operator tests; a plain fp32 conv2d weight gradient on the CPU is within
      8e-8 .. 2.1e-6 of float64 at these shapes), run twice and bit-identical (the reduce is
      fixed-order).  This leg catches a precision downgrade, which small integers survive.

Each case states which kernel it is there for -- K loop (GENERIC / FP32 / FP32_PAIRS), tile, split count
and so the form of the reduce launch, WALIGN (the launcher takes it when Wo % 16 == 0), in_affine --
and asserts that from gs_debug_last_conv_launch.  tests/test_c_abi.py checks the same table against
gs_debug_query_conv_launch without a GPU and asserts the coverage sets over the whole table.

GS_NO_FAST, GS_NO_WALIGN, GS_WGRAD_OLD_PLAN and the planner's tuning variables are read once by the
library: the tests change none of them and adjust their claims to what is set."""
import ctypes
import os
from typing import NamedTuple, Optional, Tuple, Union

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
BK = 16                    # pixels per K step (csrc/igemm_core.h)
AFF_MAX_C = 640            # kAffMaxC

NO_FAST = os.environ.get("GS_NO_FAST") is not None
NO_WALIGN = bool(int(os.environ.get("GS_NO_WALIGN") or 0))
# anything that moves the planner's natural choice (tile, split count, paired loop): the natural-plan
# claims are then checked against the host query only
PLAN_ENV = any(os.environ.get(v) for v in ("GS_WGRAD_OLD_PLAN", "GS_WG_TARGET", "GS_FORCE_BM", "GS_BN_CAP",
                                            "GS_MIN_KSTEPS", "GS_PAIR_MIN", "GS_SLAB_COST_PCT"))


class WCase(NamedTuple):
    n: int
    h: int
    w: int
    ci: int
    co: int
    k: Union[int, Tuple[int, int]]
    stride: int = 1
    dil: int = 1
    pad: Optional[int] = None
    ci_max: Optional[int] = None
    co_ld: Optional[int] = None
    ldx: Optional[int] = None
    ldy: Optional[int] = None
    force: Optional[Tuple[int, int, int]] = None     # gs_debug_force_plan(bm, bn, splits)
    # the coverage claim
    kloop: str = "FP32"                              # GEN | FP32 | PAIRS
    bm: int = 64
    bn: int = 32
    splits: int = 1
    per: Optional[int] = None                        # K steps per split
    walign: bool = False                             # Wo % 16 == 0
    aff: bool = False

    def id(self):
        k = self.k if isinstance(self.k, int) else "%dx%d" % self.k
        s = "%dx%dx%dx%dx%d-k%s" % (self.n, self.h, self.w, self.ci, self.co, k)
        if self.stride != 1:
            s += "-s%d" % self.stride
        if self.dil != 1:
            s += "-d%d" % self.dil
        if self.pad is not None:
            s += "-p%d" % self.pad
        if self.ldx is not None:
            s += "-wide"
        if self.force:
            s += "-force%dx%dx%d" % self.force
        return s


# ---- natural plans: what the planner picks on 256 CUs (gs_debug_query_conv_launch) ----
NATURAL_CASES = [
    # 1x1, WALIGN, one row tile without a ragged edge
    WCase(2, 16, 16, 64, 48, 1, kloop="FP32", bn=32, splits=8, per=4, walign=True),
    # 3x3, general loader, ragged K (442 pixels) and ragged M (432 rows)
    WCase(2, 13, 17, 48, 48, 3, kloop="FP32", bn=32, splits=7),
    # stride 2 with WALIGN (Wo = 16)
    WCase(2, 32, 32, 64, 64, 3, stride=2, kloop="FP32", bn=32, splits=8, walign=True),
    # stride 2, odd sizes, general loader (Wo = 17)
    WCase(2, 15, 33, 32, 64, 3, stride=2, kloop="FP32", bn=32, splits=4, per=5),
    # dilation: padding wider than a tap
    WCase(1, 12, 12, 32, 32, 3, dil=2, kloop="FP32", bn=32, splits=2),
    WCase(1, 20, 20, 64, 64, 3, dil=4, kloop="FP32", bn=32, splits=5),
    # 2 pixels in all: one partial K step, the pixel advance jumps 16 images
    WCase(2, 1, 1, 512, 128, 1, kloop="FP32", bn=32, splits=1, per=1),
    # images smaller than a K step: a carry in every digit of the (n, h, w) advance, most taps in padding
    WCase(2, 2, 2, 64, 64, 3, kloop="FP32", bn=32, splits=1),
    WCase(2, 3, 3, 128, 64, 3, kloop="FP32", bn=32, splits=1),
    WCase(2, 6, 6, 320, 80, 3, kloop="FP32", bn=32, splits=1),
    # M = 16 (a quarter tile), 128 splits: the WIDE reduce, WALIGN
    WCase(2, 64, 128, 16, 64, 1, kloop="FP32", bn=32, splits=128, per=8, walign=True),
    # paired K loop + WALIGN + WIDE reduce, 64-column tile
    WCase(2, 64, 128, 64, 256, 1, kloop="PAIRS", bn=64, splits=64, per=16, walign=True),
    # paired K loop with an odd step count, sequential reduce of 14 slabs
    WCase(2, 32, 64, 64, 64, 3, kloop="PAIRS", bn=32, splits=14, per=19, walign=True),
    # paired K loop, general loader, 16 column tiles, ragged last split
    WCase(2, 33, 33, 256, 1024, 1, kloop="PAIRS", bn=64, splits=4, per=35),
    # paired K loop, unsplit (direct o_tap / o_row store), widest operand
    WCase(2, 17, 17, 640, 160, 3, kloop="PAIRS", bn=32, splits=1, per=37),
    # 48-column tile, unsplit
    WCase(2, 8, 8, 512, 128, 3, kloop="FP32", bn=48, splits=1),
    # 64-column tile, unsplit, 32 row tiles
    WCase(2, 9, 9, 2048, 512, 1, kloop="FP32", bn=64, splits=1),
    # KS = 0 fast kernel (runtime KW), non-square taps
    WCase(2, 32, 40, 8, 32, 7, stride=2, kloop="FP32", bn=32, splits=10),
    WCase(1, 20, 24, 16, 32, 5, kloop="FP32", bn=32, splits=6),
    WCase(1, 20, 24, 32, 32, (1, 3), pad=0, kloop="FP32", bn=32, splits=7),
    # generic SCALAR kernel (x_sw not a multiple of 4): the four rows of a thread lie in different taps
    WCase(2, 17, 19, 6, 24, 3, kloop="GEN", bn=32, splits=9),
    WCase(2, 17, 19, 3, 24, 3, stride=2, kloop="GEN", bn=32, splits=3),
    # every pitch wider than its extent
    WCase(2, 12, 20, 48, 80, 3, ci_max=64, co_ld=96, ldx=64, ldy=96, kloop="FP32", bn=32, splits=6),
    # strided 1x1 shortcut
    WCase(2, 15, 15, 64, 256, 1, stride=2, pad=0, kloop="FP32", bn=32, splits=2),
    # Co = 20 (a padded class conv): one 32-wide tile with 12 dead columns
    WCase(2, 9, 11, 64, 20, 1, kloop="FP32", bn=32, splits=3),
]

# ---- forced plans: the tiles only gs_debug_force_plan reaches (tools/sweep_conv_plans.py) ----
# 3x3 on 2 x 20 x 24, 96 -> 176: M = 864 (ragged for 64 and for 128 rows), a ragged last column tile at
# every width; 960 pixels = 60 K steps
_F = dict(n=2, h=20, w=24, ci=96, co=176, k=3)
FORCED_CASES = (
    [WCase(**_F, force=(128, bn, 5), kloop="FP32", bm=128, bn=bn, splits=5, per=12) for bn in (128, 96, 80, 64, 48, 32)] +
    [WCase(**_F, force=(64, bn, 5), kloop="FP32", bm=64, bn=bn, splits=5, per=12) for bn in (80, 64, 48)] +
    [WCase(**_F, force=(64, 80, 1), kloop="PAIRS", bm=64, bn=80, splits=1, per=60),       # paired, unsplit
     WCase(**_F, force=(64, 64, 20), kloop="FP32", bm=64, bn=64, splits=20, per=3),       # WIDE reduce, 3-step splits
     # 128 rows, WALIGN and the WIDE reduce together: 43 splits of 3 steps and a last one of 2
     WCase(2, 32, 32, 96, 176, 3, force=(128, 64, 60), kloop="FP32", bm=128, bn=64, splits=43, per=3, walign=True)] +
    # the 128-row tiles on a 1x1 with Wo % 16 == 0: both register slots of the WALIGN loader
    [WCase(2, 16, 32, 160, 176, 1, force=(128, bn, 5), kloop="FP32", bm=128, bn=bn, splits=5, per=13, walign=True)
     for bn in (128, 96, 80, 64, 48, 32)]
)

# ---- in_affine: relu(bn(x)) evaluated in the operand loader ----
AFF_CASES = [
    WCase(2, 16, 32, 64, 64, 3, aff=True, kloop="FP32", bn=32, splits=13, per=5, walign=True),  # 3x3 WALIGN
    WCase(2, 15, 33, 32, 64, 3, stride=2, aff=True, kloop="FP32", bn=32, splits=4, per=5),  # stride 2, general loader
    WCase(1, 20, 20, 64, 64, 3, dil=4, aff=True, kloop="FP32", bn=32, splits=5),            # dilated
    WCase(2, 9, 9, AFF_MAX_C, 64, 1, aff=True, kloop="FP32", bn=32, splits=2, per=6),       # Ci at the limit
    WCase(2, 32, 64, 64, 64, 3, aff=True, kloop="PAIRS", bn=32, splits=14, per=19, walign=True),
]

ALL_CASES = NATURAL_CASES + FORCED_CASES + AFF_CASES
KLOOPS = {"GEN": 0, "FP32": 1, "PAIRS": 2}       # lib.KLOOP_GENERIC / _FP32 / _FP32_PAIRS


def make_desc(lib, c):
    return lib.conv_desc(c.n, c.h, c.w, c.ci, c.co, c.k, stride=c.stride, dil=c.dil, pad=c.pad,
                         ci_max=c.ci_max, co_ld=c.co_ld, ldx=c.ldx, ldy=c.ldy)


def is_vector(c):
    """the fast kernels' source condition (x_is_vector): float4 loads of an NHWC x"""
    return c.ci % 4 == 0 and (c.ldx or c.ci) % 4 == 0


def reduce_form(splits, m, co):
    """launch_reduce: none | seq (one thread walks the slabs) | wide (16 slab groups through LDS)"""
    if splits <= 1:
        return "none"
    return "wide" if splits >= 48 or (splits >= 16 and m * (co // 4) < 65536) else "seq"


def expected_kloop(c):
    return KLOOPS["GEN"] if NO_FAST or not is_vector(c) else KLOOPS[c.kloop]


def check_claim(c, d, rec):
    """the record (of a launch, or of the host query) against the case's coverage claim"""
    from gaia_seg_amd.hip import lib
    assert rec.op == lib.OP_WGRAD
    assert rec.in_affine == (1 if c.aff else 0)
    assert (d.Wo % BK == 0) == c.walign, "the case's WALIGN claim does not follow from its shape"
    nk = -(-c.n * d.Ho * d.Wo // BK)
    assert rec.splits >= 1 and rec.splits * rec.ksteps_per_split >= nk > (rec.splits - 1) * rec.ksteps_per_split
    if c.force:
        assert (rec.bm, rec.bn) == c.force[:2] == (c.bm, c.bn)
        assert (rec.splits, rec.ksteps_per_split) == (c.splits, c.per)
        if not PLAN_ENV:
            assert rec.kloop == expected_kloop(c)
        return
    if PLAN_ENV:
        assert rec.kloop == KLOOPS["GEN"] if (NO_FAST or not is_vector(c)) else rec.kloop in (1, 2)
        return
    assert rec.kloop == expected_kloop(c)
    assert (rec.bm, rec.bn, rec.splits) == (c.bm, c.bn, c.splits)
    if c.per is not None:
        assert rec.ksteps_per_split == c.per


class forced_plan:
    """gs_debug_force_plan for the case's launches and queries, always reset"""
    def __init__(self, hip_lib, c):
        self.L, self.force = hip_lib, c.force

    def __enter__(self):
        if self.force:
            assert self.L.gs_debug_force_plan(*self.force) == 0

    def __exit__(self, *exc):
        if self.force:
            self.L.gs_debug_force_plan(0, 0, 0)


# ------------------------------------------------------------------------------------------
# data and reference
# ------------------------------------------------------------------------------------------
def small_ints(gen, *shape):
    """nonzero integers in {+-1, +-2, +-3}"""
    return (torch.randint(1, 4, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def make_inputs(lib, c, exact, seed):
    """x [n, h, w, ci], dy [n, ho, wo, co] and, for an in_affine case, the coefficient block
    [scale | beta | mean | invstd] x ci"""
    d = make_desc(lib, c)
    gen = torch.Generator().manual_seed(seed)
    if exact:
        x, dy = small_ints(gen, c.n, c.h, c.w, c.ci), small_ints(gen, c.n, d.Ho, d.Wo, c.co)
    else:
        x, dy = torch.randn(c.n, c.h, c.w, c.ci, generator=gen), torch.randn(c.n, d.Ho, d.Wo, c.co, generator=gen)
    coeffs = None
    if c.aff:
        if exact:
            # integer mean and beta, scale in {0.5, 1, 2}: the activation is a multiple of 0.5 below 12,
            # the sums stay exact; beta - mean * scale > 0 on most channels, so a padded tap that went
            # through the BatchNorm would not be zero
            scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.ci,), generator=gen)]
            beta = torch.randint(1, 4, (c.ci,), generator=gen).float()
            mean = torch.randint(-1, 2, (c.ci,), generator=gen).float()
        else:
            scale, beta, mean = (torch.randn(c.ci, generator=gen) for _ in range(3))
        invstd = torch.rand(c.ci, generator=gen) + 0.5          # not read by the loaders
        coeffs = torch.cat([scale, beta, mean, invstd])
    return x, dy, coeffs


def reference(lib, c, x, dy, coeffs=None):
    """float64 weight gradient on the CPU as [kh, kw, ci, co]"""
    d = make_desc(lib, c)
    kh, kw = c.k if isinstance(c.k, tuple) else (c.k, c.k)
    a = x.double()
    if coeffs is not None:
        scale, beta, mean = (coeffs[i * c.ci:(i + 1) * c.ci].double() for i in range(3))
        a = F.relu((a - mean) * scale + beta)            # zero padding applies to the activation
    wz = torch.zeros(c.co, c.ci, kh, kw, dtype=torch.float64, requires_grad=True)
    F.conv2d(a.permute(0, 3, 1, 2), wz, None, c.stride, d.pad, c.dil).backward(dy.double().permute(0, 3, 1, 2))
    return wz.grad.permute(2, 3, 1, 0).contiguous()


# ------------------------------------------------------------------------------------------
# the launch helper
# ------------------------------------------------------------------------------------------
class Launch:
    """Device buffers of one gs_conv2d_wgrad call under the rules of the module docstring."""

    def __init__(self, hip_lib, lib, c, x, dy, coeffs=None, workspace=None):
        self.L, self.lib, self.c = hip_lib, lib, c
        self.d = d = make_desc(lib, c)
        ldx, ldy = c.ldx or c.ci, c.ldy or c.co
        xg = torch.full((c.n, c.h, c.w, ldx), float("nan"))
        xg[..., :c.ci] = x
        dyg = torch.full((c.n, d.Ho, d.Wo, ldy), float("nan"))
        dyg[..., :c.co] = dy
        self.x, self.dy = xg.to(DEV), dyg.to(DEV)
        self.coeffs = None if coeffs is None else coeffs.to(DEV)
        if self.coeffs is not None:
            assert self.coeffs.data_ptr() % 16 == 0
            d.in_affine = self.coeffs.data_ptr()
            assert hip_lib.gs_conv2d_in_affine_supported(ctypes.byref(d)) == 1, "pick another shape"
        self.dw = torch.full((d.KH, d.KW, d.Ci_max, d.Co_ld), SENTINEL, device=DEV)
        self.need = hip_lib.gs_conv2d_workspace_bytes(ctypes.byref(d))
        self.own_ws = workspace is None
        if self.own_ws:       # exactly `need` bytes of NaN, then the guard
            workspace = torch.empty(self.need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
            workspace[:self.need] = 0xFF
            workspace[self.need:] = GUARD_BYTE
        self.ws = workspace

    def issue(self):
        from gaia_seg_amd.hip.runtime import current_stream_ptr
        self.lib.check(self.L.gs_conv2d_wgrad(ctypes.byref(self.d), self.x.data_ptr(), self.dy.data_ptr(),
                                              self.dw.data_ptr(), self.ws.data_ptr(), self.need,
                                              current_stream_ptr()), "wgrad")
        self.rec = self.lib.DebugLaunch()
        assert self.L.gs_debug_last_conv_launch(ctypes.byref(self.rec)) == 0
        return self

    def result(self):
        """synchronise, check everything around the active slice, return it on the CPU"""
        c = self.c
        torch.cuda.synchronize()
        dw = self.dw.cpu()
        outside = torch.ones_like(dw, dtype=torch.bool)
        outside[:, :, :c.ci, :c.co] = False
        assert bool((dw[outside] == SENTINEL).all()), "a store outside [:, :, :Ci, :Co]"
        if self.own_ws:
            assert bool((self.ws[self.need:] == GUARD_BYTE).all()), "the slab overran the workspace"
        active = dw[:, :, :c.ci, :c.co].contiguous()
        assert bool(torch.isfinite(active).all()), "NaN: an unwritten slab cell or a pad column was read"
        return active


def run_case(hip_lib, lib, c, x, dy, coeffs=None):
    """one synchronised launch (forced plan included): (active dw slice on the CPU, launch record)"""
    with forced_plan(hip_lib, c):
        run = Launch(hip_lib, lib, c, x, dy, coeffs).issue()
        q = lib.DebugLaunch()
        assert hip_lib.gs_debug_query_conv_launch(ctypes.byref(run.d), lib.OP_WGRAD, ctypes.byref(q)) == 0
    got = run.result()
    assert bytes(q) == bytes(run.rec), "the host query and the launch disagree"
    check_claim(c, run.d, run.rec)
    return got, run.rec


def check_both_legs(hip_lib, c):
    from gaia_seg_amd.hip import lib
    # (a) exact
    x, dy, coeffs = make_inputs(lib, c, True, 11)
    got, rec = run_case(hip_lib, lib, c, x, dy, coeffs)
    want = reference(lib, c, x, dy, coeffs)
    print("%s: kloop %d tile %dx%d splits %d x %d steps, in_affine %d, max |dw| %g" % (
        c.id(), rec.kloop, rec.bm, rec.bn, rec.splits, rec.ksteps_per_split, rec.in_affine,
        float(want.abs().max())))
    assert float(want.abs().max()) < 2 ** 22
    assert torch.equal(got.double(), want), "exact leg: %d of %d elements differ, largest by %g" % (
        int((got.double() != want).sum()), want.numel(), float((got.double() - want).abs().max()))
    # (b) random, twice
    x, dy, coeffs = make_inputs(lib, c, False, 12)
    first, _ = run_case(hip_lib, lib, c, x, dy, coeffs)
    second, _ = run_case(hip_lib, lib, c, x, dy, coeffs)
    err = rel_err(first, reference(lib, c, x, dy, coeffs))
    print("%s: random leg rel_err %.3g" % (c.id(), err))
    assert err < TOL
    assert torch.equal(first, second), "two runs of the same input differ"


@pytest.mark.parametrize("case", NATURAL_CASES, ids=WCase.id)
def test_natural_plans(hip_lib, case):
    check_both_legs(hip_lib, case)


@pytest.mark.parametrize("case", FORCED_CASES, ids=WCase.id)
def test_forced_tiles(hip_lib, case):
    check_both_legs(hip_lib, case)


@pytest.mark.parametrize("case", AFF_CASES, ids=WCase.id)
def test_in_affine(hip_lib, case):
    if NO_FAST:
        pytest.skip("in_affine needs the fast kernels (GS_NO_FAST is set)")
    check_both_legs(hip_lib, case)


def test_walign_loader_equals_the_general_loader_bit_for_bit(hip_lib):
    """A 1x1 weight gradient depends only on the order of the pixels.  The same packed x / dy memory
    read as four (n, h, w) geometries of 512 pixels -- two with Wo % 16 == 0 (the WALIGN loader), two
    without (the general one, its (n, h, w) advance carrying in different digits) -- has the same M, N
    and K, hence the same plan and the same summation order: the four dw are bit-identical."""
    from gaia_seg_amd.hip import lib
    ci = co = 64
    gen = torch.Generator().manual_seed(21)
    x, dy = torch.randn(512, ci, generator=gen), torch.randn(512, co, generator=gen)
    outs, plans, waligns = [], set(), []
    for n, h, w in [(2, 8, 32), (2, 32, 8), (1, 64, 8), (4, 1, 128)]:
        c = WCase(n, h, w, ci, co, 1)
        run = Launch(hip_lib, lib, c, x.view(n, h, w, ci), dy.view(n, h, w, co)).issue()
        outs.append(run.result())
        rec = run.rec
        assert rec.op == lib.OP_WGRAD
        plans.add((rec.kloop, rec.bm, rec.bn, rec.splits, rec.ksteps_per_split))
        waligns.append(w % BK == 0)
    assert waligns == [True, False, False, True]
    assert len(plans) == 1, plans
    want = (x.double().t() @ dy.double()).view(1, 1, ci, co)
    assert rel_err(outs[0], want) < TOL
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_back_to_back_launches_on_one_stream(hip_lib):
    """30 launches on one stream without host synchronisation, three shapes alternating on ONE workspace
    (each launch's slabs overlap the previous launch's: 14 sequentially reduced slabs, 7 ragged ones,
    128 for the WIDE reduce), new inputs every launch.  Each result equals a synchronised single
    launch of the same input bit for bit: the reduce of launch i has finished with the slabs before
    launch i + 1 rewrites them, and reads nothing that launch i - 1 left there.  (The single launch
    itself is held against float64, so that the comparison is not of the code with itself alone.)"""
    from gaia_seg_amd.hip import lib
    shapes = [NATURAL_CASES[12], NATURAL_CASES[1], NATURAL_CASES[10]]
    assert [s.splits for s in shapes] == [14, 7, 128]
    need = max(hip_lib.gs_conv2d_workspace_bytes(ctypes.byref(make_desc(lib, s))) for s in shapes)
    shared = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)
    shared[:need] = 0xFF
    shared[need:] = GUARD_BYTE
    runs = []
    for i in range(30):
        c = shapes[i % 3]
        x, dy, _ = make_inputs(lib, c, False, 100 + i)
        runs.append((x, dy, Launch(hip_lib, lib, c, x, dy, workspace=shared)))
    torch.cuda.synchronize()
    for _, _, run in runs:           # nothing but the 30 launches (and their reduces) on the stream
        run.issue()
    torch.cuda.synchronize()
    assert bool((shared[need:] == GUARD_BYTE).all())
    for i, (x, dy, run) in enumerate(runs):
        c = shapes[i % 3]
        got = run.result()
        if not PLAN_ENV and not NO_FAST:
            assert run.rec.splits == c.splits
        alone, _ = run_case(hip_lib, lib, c, x, dy)
        assert torch.equal(got, alone), i
        assert rel_err(alone, reference(lib, c, x, dy)) < TOL, i
