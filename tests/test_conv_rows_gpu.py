"""The convolution forward and data gradient through the C-ABI (gs_conv2d_forward, gs_conv2d_dgrad;
csrc/igemm_fwd.hip, csrc/igemm_dgrad.hip, the row kernels igemm_rows_fast_kernel / igemm_rows_kernel /
splitk_reduce_kernel of csrc/igemm_core.h), under the protocol of tests/test_wgrad_gpu.py.

Every case runs on buffers that forgive nothing:

  * the output (y, or dx) is allocated at its pitch plus GUARD_ROWS rows and pre-filled with a
    sentinel: everything outside [rows, :Co] (resp. [rows, :Ci]) must still hold it afterwards -- with
    accumulate = 1 as well -- and the active part must be finite;
  * x, dy and the addend hold NaN in every column past their extent when their pitch is wider;
  * the weight [KH][KW][Ci_max][Co_ld] holds 2^20 outside [:, :, :Ci, :Co]: a kernel that masks the
    OTHER operand to zero still passes (0 * 2^20 = 0), one that really contracts over the inactive slice
    fails both legs.  The two NANW cases (a ragged last K step of the generic kernels: Ci = 24 of
    Ci_max = 32 forward, Co = 20 of Co_ld = ldy = 32 data gradient) hold NaN there instead: pad columns of
    a concat slice belong to another tensor, and 0 * NaN would not be 0;
  * the workspace is exactly gs_conv2d_workspace_bytes(d) bytes of 0xFF (NaN) in front of a 4 KiB guard
    pattern: a slab cell read before it was written turns the result NaN, an overrun breaks the guard.
    (The query is the maximum over the three ops: what lies between this op's own slabs and the end of
    the workspace must still be 0xFF, too.)

and with two kinds of data:

  (a) exact: x / dy, w, bias, addend and the accumulate base are nonzero integers in {+-1, +-2, +-3}
      (in_affine: the scale / beta / mean trick of test_wgrad_gpu.make_inputs, an activation that is a
      multiple of 0.5 below 12).  Every product and partial sum is an integer (or a half) far below
      2^22 -- asserted per case; the largest here is 9 * 9 * 640 = 51840 --, so fp32 accumulation is
      exact in any order, under any split count and either form of the reduce: torch.equal against
      float64.  One dropped, duplicated or misplaced tap or pixel moves an element by at least 1, and
      the failure message counts the differing elements.
  (b) random: standard normal data against float64 F.conv2d (+ bias + addend) or its autograd input
      gradient within TOL = 3e-5, the bound of the exact-fp32-MFMA operator tests, run twice and
      bit-identical.  A plain float32 conv on the CPU is within 1.5e-7 .. 2.6e-6 (forward) and
      1.5e-7 .. 6.5e-7 (input gradient) of float64 over the shapes of this table (measured on the CPU,
      against the float64 reference, not against the kernels): TOL has a margin of 11x over summation
      order alone, and an fp16 operand rounding (5e-4) is 16x outside it.

Every data-gradient case runs three times per leg: dx = plain, and dx += onto a base, which must equal
base + plain exactly in (a) and lie within TOL of the float64 sum in (b).

Each case claims what it is there for, per op, as `<K loop> <bm>x<bn> x<splits> [launch|reduce] [aff]
[classes]`: the K loop (GEN / FP32 / PAIRS), the tile, the split count, whether the slabs are combined
inside the launch (splitk_publish; counted by gs_debug_splitk_combined) or by the separate
splitk_reduce_kernel launch, in_affine, and whether a strided data gradient runs as parity classes
(dgrad_strided_fast).  The claim is asserted against gs_debug_last_conv_launch after the launch and
against gs_debug_query_conv_launch, which must agree byte for byte; tests/test_c_abi.py checks the same
table without a GPU and asserts the coverage sets over the whole table.  For a data gradient in parity
classes the header says that the query describes class (0, 0) and the record the LAST class launched,
whose row and tap counts differ: there each is held, byte for byte, against the plan of its own class
(gs_debug_query_plan of the class's M x Ci x taps * Co, the K loop by pair_loop_ok's rule).
No case lands on the stem, streaming, bf16x3 or f16 paths (asserted): they have files of their own.

The groups and the kernels / template parameters they are there for:

  NATURAL   the planner's own plans.  igemm_rows_fast_kernel<64, 32|48|64|80, BTRANS = false|true,
            KS = 1|3, KLOOP = FP32|FP32_PAIRS, SK = false|true>: unsplit and split (in-launch combine),
            ragged M, dilation (padding wider than a tap), two rows, images smaller than a K step,
            every pitch wider than its extent, tile_order 0 and 1.
  EPILOGUE  forward bias / addend: rows_epilogue on dead tile columns (Co = 20), ld_add > Co with
            ldy > Co, and bias + addend through the in-launch combine.
  GENERIC   igemm_rows_kernel<64, BN, BTRANS, DIVS, SCALAR = false, KS = 0|1|3>: a vector source that
            is not fast (channels % 16 != 0, or taps other than 1x1 / 3x3), K steps that straddle taps,
            a ragged last K step, splitk_reduce_kernel behind it; DIVS = true: the strided data
            gradient with Co % 16 != 0 (KS = 3) or other taps (KS = 0).
  SCALAR    igemm_rows_kernel<.., SCALAR = true, KS = 0> (forward only): x_sw % 4 != 0, and an
            NCHW-strided x the stem gate refuses.
  STRIDED   dgrad_strided_fast: one fast launch per parity class through the o_s / o_ph / o_pw output
            lattice; odd image sizes (class_len), stride 3, classes without a tap cleared by
            hipMemsetAsync (dense dx) or zero_rows_kernel (sliced dx) and left alone under +=, tapless
            odd classes inside a dilated 3x3.
  AFFINE    igemm_rows_fast_kernel<64, BN, false, KS, ROLE, FP32|FP32_PAIRS, AFF = true>: relu(bn(x)) in
            the loader, zero padding applied to the activation.
  FORCED    gs_debug_force_plan on 2 x 20 x 24, 96 -> 176, 3x3 (M = 960: ragged for 128 rows, a ragged
            last column tile at every width): igemm_rows_fast_kernel<128|64, 128|96|80|64|48|32, ..>
            unsplit and split, both fp32 loops on either row height, splitk_reduce_kernel with bias +
            addend / accumulate behind tiles that cannot combine in the launch.

GS_NO_FAST, GS_SPLITK_INKERNEL and the planner's tuning variables are read once by the library: the
tests change none of them and adjust their claims to what is set."""
import ctypes
import functools
import os
from typing import NamedTuple, Optional, Tuple, Union

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_wgrad_gpu import AFF_MAX_C, BK, GUARD_BYTE, GUARD_BYTES, SENTINEL, TOL, forced_plan, small_ints

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ROWS = 3
POISON = float(2 ** 20)
EXACT_BOUND = 2 ** 22

NO_FAST = os.environ.get("GS_NO_FAST") is not None
NO_COMBINE = os.environ.get("GS_SPLITK_INKERNEL", "1") == "0"
# anything that moves the planner's natural choice (tile, split count, K loop): the natural-plan claims
# are then checked against the host query only
PLAN_ENV = any(os.environ.get(v) for v in ("GS_X3", "GS_STREAM", "GS_FORCE_BM", "GS_WG_TARGET", "GS_MIN_KSTEPS",
                                            "GS_PAIR_MIN", "GS_SLAB_COST_PCT", "GS_BN_CAP"))
KNAMES = {0: "GEN", 1: "FP32", 2: "PAIRS"}         # lib.KLOOP_GENERIC / _FP32 / _FP32_PAIRS: all this file admits
FWD, DGRAD = "fwd", "dgrad"


class CCase(NamedTuple):
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
    ld_add: Optional[int] = None                     # pitch of the addend (default Co)
    bias: bool = False
    addend: bool = False
    aff: bool = False
    nchw: bool = False                               # x is an NCHW image (x_sc = H * W)
    nan_w: bool = False                              # NaN instead of 2^20 around the weight slice
    force: Optional[Tuple[int, int, int]] = None     # gs_debug_force_plan(bm, bn, splits)
    # the coverage claims (None: the op does not run on this case)
    fwd: Optional[str] = None
    dgr: Optional[str] = None

    def id(self):
        k = self.k if isinstance(self.k, int) else "%dx%d" % self.k
        s = "%dx%dx%dx%dx%d-k%s" % (self.n, self.h, self.w, self.ci, self.co, k)
        if self.stride != 1:
            s += "-s%d" % self.stride
        if self.dil != 1:
            s += "-d%d" % self.dil
        if self.pad is not None:
            s += "-p%d" % self.pad
        if self.ldx is not None or self.ldy is not None or self.ci_max is not None:
            s += "-wide"
        for flag in ("bias", "addend", "aff", "nchw", "nan_w"):
            if getattr(self, flag):
                s += "-" + flag
        if self.force:
            s += "-force%dx%dx%d" % self.force
        return s

    def claim(self, op):
        return self.fwd if op == FWD else self.dgr


C = CCase
# ---- natural plans, both ops: what the planner picks on 256 CUs (gs_debug_query_conv_launch) ----
NATURAL_CASES = [
    # 1x1, one 32-column tile pair, no ragged edge
    C(2, 16, 16, 64, 48, 1, fwd="FP32 64x32 x1", dgr="FP32 64x32 x1"),
    # 3x3, ragged M (442 rows) and K, split and combined in the launch
    C(2, 13, 17, 48, 48, 3, fwd="FP32 64x32 x6 launch", dgr="FP32 64x32 x6 launch"),
    # dilation: padding wider than a tap
    C(1, 12, 12, 32, 32, 3, dil=2, fwd="FP32 64x32 x4 launch", dgr="FP32 64x32 x4 launch"),
    C(1, 20, 20, 64, 64, 3, dil=4, fwd="FP32 64x32 x9 launch", dgr="FP32 64x32 x9 launch"),
    # two rows in all
    C(2, 1, 1, 512, 128, 1, fwd="FP32 64x32 x8 launch", dgr="FP32 64x32 x2 launch"),
    # images smaller than a K step: most taps in padding
    C(2, 2, 2, 64, 64, 3, fwd="FP32 64x32 x9 launch", dgr="FP32 64x32 x9 launch"),
    C(2, 3, 3, 128, 64, 3, fwd="FP32 64x32 x18 launch", dgr="FP32 64x32 x9 launch"),
    # every pitch wider than its extent
    C(2, 12, 20, 48, 80, 3, ci_max=64, co_ld=96, ldx=64, ldy=96,
      fwd="FP32 64x32 x6 launch", dgr="FP32 64x32 x9 launch"),
    # the paired K loop, widest operand; 64-column tile on the data gradient
    C(2, 17, 17, 640, 160, 3, fwd="PAIRS 64x32 x15 launch", dgr="PAIRS 64x64 x5 launch"),
    # the paired K loop unsplit, 16 / 4 column tiles
    C(2, 33, 33, 256, 1024, 1, fwd="PAIRS 64x80 x1", dgr="FP32 64x64 x5 launch"),
    # deep splits
    C(2, 8, 8, 512, 128, 3, fwd="FP32 64x32 x32 launch", dgr="FP32 64x32 x8 launch"),
    # 64-column tile, the weight the larger operand (tile_order 1)
    C(2, 9, 9, 2048, 512, 1, fwd="FP32 64x64 x10 launch", dgr="FP32 64x32 x4 launch"),
]

# ---- the forward epilogue ----
EPILOGUE_CASES = [
    # Co = 20 (a padded class conv): 12 dead tile columns under the bias; its data gradient is generic
    C(2, 9, 11, 64, 20, 1, bias=True, fwd="FP32 64x32 x1", dgr="GEN 64x32 x1"),
    # addend at its own pitch beside a wider y
    C(2, 12, 20, 48, 80, 3, ci_max=64, co_ld=96, ldx=64, ldy=96, ld_add=88, addend=True,
      fwd="FP32 64x32 x6 launch"),
    # bias + addend through the in-launch combine
    C(2, 13, 17, 48, 48, 3, bias=True, addend=True, fwd="FP32 64x32 x6 launch"),
    # the ragged last K step of the generic data gradient beside NaN: dy columns 20..31, weight columns 20..31
    C(2, 9, 11, 64, 20, 1, co_ld=32, ldy=32, nan_w=True, dgr="GEN 64x32 x1"),
]

# ---- the generic vector kernels ----
GENERIC_CASES = [
    C(2, 9, 9, 24, 48, 3, fwd="GEN 64x32 x3 reduce", dgr="FP32 64x32 x6 launch"),
    C(2, 9, 9, 48, 24, 3, fwd="FP32 64x32 x6 launch", dgr="GEN 64x32 x3 reduce"),
    C(2, 9, 9, 40, 40, 1, fwd="GEN 64x32 x1", dgr="GEN 64x32 x1"),
    # the ragged last K step of the generic forward beside NaN: weight rows 24..31
    C(2, 9, 9, 24, 48, 3, ci_max=32, nan_w=True, fwd="GEN 64x32 x3 reduce"),
    # runtime KW
    C(1, 20, 24, 16, 32, 5, fwd="GEN 64x32 x5 reduce", dgr="GEN 64x32 x10 reduce"),
    C(1, 20, 24, 32, 32, (1, 3), pad=0, fwd="GEN 64x32 x1", dgr="GEN 64x32 x1"),
    # DIVS with KS = 0: the patch-embedding / downsampling convs of ConvNeXt, Swin and MiT
    C(2, 32, 40, 8, 32, 7, stride=2, fwd="GEN 64x32 x5 reduce", dgr="GEN 64x32 x6 reduce"),
    C(2, 14, 18, 96, 192, 2, stride=2, pad=0, fwd="GEN 64x32 x6 reduce", dgr="GEN 64x32 x10 reduce"),
    C(2, 16, 24, 32, 64, 4, stride=4, pad=0, fwd="GEN 64x32 x8 reduce", dgr="GEN 64x32 x16 reduce"),
    C(1, 16, 16, 64, 64, 8, stride=8, pad=0, fwd="GEN 64x32 x64 reduce", dgr="GEN 64x32 x32 reduce"),
    C(2, 32, 40, 64, 32, 7, stride=4, pad=3, fwd="GEN 64x32 x49 reduce", dgr="GEN 64x64 x6 reduce"),
    # DIVS with KS = 3: Co % 16 != 0
    C(2, 16, 16, 48, 24, 3, stride=2, fwd="FP32 64x32 x6 launch", dgr="GEN 64x32 x3 reduce"),
]

# ---- the generic scalar kernel (forward only: the data gradient needs Ci % 4 == 0, x_sc == 1) ----
SCALAR_CASES = [
    C(2, 17, 19, 6, 24, 3, fwd="GEN 64x32 x1"),
    C(2, 17, 19, 3, 24, 3, stride=2, fwd="GEN 64x32 x1"),
    # an NCHW image that is not the stem's (3x3; Wo = 19 is no multiple of 128)
    C(2, 17, 19, 3, 24, 3, nchw=True, fwd="GEN 64x32 x1"),
]

# ---- the strided data gradient as parity classes ----
STRIDED_CASES = [
    C(2, 16, 16, 64, 64, 3, stride=2, fwd="FP32 64x32 x9 launch", dgr="FP32 64x32 x1 classes"),
    # odd sizes: the classes differ in rows and columns
    C(2, 15, 33, 32, 64, 3, stride=2, fwd="FP32 64x32 x4 launch", dgr="FP32 64x32 x1 classes"),
    # three classes without a tap: dense dx (hipMemsetAsync) and sliced dx (zero_rows_kernel)
    C(2, 15, 15, 64, 256, 1, stride=2, pad=0, fwd="FP32 64x32 x1", dgr="FP32 64x32 x4 launch classes"),
    C(2, 15, 15, 64, 256, 1, stride=2, pad=0, ldx=80, dgr="FP32 64x32 x4 launch classes"),
    # stride 2 under dilation 2: the odd classes have no tap, the even ones all nine
    C(2, 16, 16, 64, 64, 3, stride=2, dil=2, fwd="FP32 64x32 x9 launch", dgr="FP32 64x32 x9 launch classes"),
    C(2, 17, 17, 64, 64, 3, stride=3, fwd="FP32 64x32 x9 launch", dgr="FP32 64x32 x1 classes"),
]

# ---- in_affine (forward): relu(bn(x)) evaluated in the operand loader ----
AFF_CASES = [
    C(2, 16, 32, 64, 64, 3, aff=True, fwd="FP32 64x32 x8 launch aff"),
    C(2, 15, 33, 32, 64, 3, stride=2, aff=True, fwd="FP32 64x32 x4 launch aff"),
    C(1, 20, 20, 64, 64, 3, dil=4, aff=True, fwd="FP32 64x32 x9 launch aff"),
    C(2, 9, 9, AFF_MAX_C, 64, 1, aff=True, fwd="FP32 64x32 x10 launch aff"),
    C(2, 32, 64, 64, 64, 3, aff=True, fwd="PAIRS 64x32 x2 launch aff"),
    C(2, 9, 9, 64, 64, 1, stride=2, pad=0, aff=True, fwd="FP32 64x32 x1 aff"),
]

# ---- forced plans: the tiles only gs_debug_force_plan reaches ----
# 3x3 on 2 x 20 x 24, 96 -> 176: M = 960 (ragged for 128 rows), a ragged last column tile at every
# width.  Forward: 54 K steps (unsplit: PAIRS; 5 splits of 11: FP32).  Data gradient: 99 K steps
# (unsplit and 5 splits of 20: PAIRS; 9 splits of 11: FP32).
_F = dict(n=2, h=20, w=24, ci=96, co=176, k=3)
_BMS, _BNS = (128, 64), (128, 96, 80, 64, 48, 32)


def _forced(op, bm, bn, splits, loop, **kw):
    combine = "" if splits == 1 else (" launch" if bm == 64 and bn <= 80 else " reduce")
    text = "%s %dx%d x%d%s" % (loop, bm, bn, splits, combine)
    return C(**_F, force=(bm, bn, splits), **kw, **{"fwd" if op == FWD else "dgr": text})


FORCED_CASES = (
    [_forced(FWD, bm, bn, 1, "PAIRS") for bm in _BMS for bn in _BNS] +
    [_forced(FWD, bm, bn, 5, "FP32") for bm in _BMS for bn in _BNS] +
    # bias + addend behind the reduce launch (tiles that cannot combine) and through the combine
    [_forced(FWD, bm, bn, 5, "FP32", bias=True, addend=True) for bm, bn in ((64, 96), (128, 64), (64, 80))] +
    [_forced(DGRAD, bm, bn, 1, "PAIRS") for bm in _BMS for bn in _BNS] +
    [_forced(DGRAD, bm, bn, 9, "FP32") for bm in _BMS for bn in _BNS] +
    [_forced(DGRAD, bm, bn, 5, "PAIRS") for bm, bn in ((64, 96), (128, 128), (64, 80))]
)

ALL_CASES = NATURAL_CASES + EPILOGUE_CASES + GENERIC_CASES + SCALAR_CASES + STRIDED_CASES + AFF_CASES + FORCED_CASES
PARAMS = [(c, op) for c in ALL_CASES for op in (FWD, DGRAD) if c.claim(op)]


def param_id(p):
    return p if isinstance(p, str) else p.id()


# ------------------------------------------------------------------------------------------
# descriptor, route and claim (host arithmetic: tests/test_c_abi.py uses these without a GPU)
# ------------------------------------------------------------------------------------------
def make_desc(lib, c):
    d = lib.conv_desc(c.n, c.h, c.w, c.ci, c.co, c.k, stride=c.stride, dil=c.dil, pad=c.pad, ci_max=c.ci_max,
                      co_ld=c.co_ld, ldx=c.ldx, ldy=c.ldy, ld_add=(c.ld_add or c.co) if c.addend else 0)
    if c.nchw:
        d.x_sn, d.x_sc, d.x_sh, d.x_sw = c.ci * c.h * c.w, c.h * c.w, c.w, 1
    return d


def is_vector(c):
    """the forward's source condition (x_is_vector): float4 loads of an NHWC x"""
    return not c.nchw and c.ci % 4 == 0 and (c.ldx or c.ci) % 4 == 0


def is_fast(c, d, op):
    """the fast row kernels' conditions (fast_rows_ok): 1x1 or 3x3, gathered channels % 16 == 0"""
    taps_ok = (d.KH, d.KW) in ((1, 1), (3, 3))
    if op == FWD:
        return not NO_FAST and is_vector(c) and taps_ok and c.ci % BK == 0
    return not NO_FAST and taps_ok and c.co % BK == 0


def gemm_dims(c, d, op):
    """M x N x K of the op's implicit GEMM"""
    taps = d.KH * d.KW
    if op == FWD:
        return c.n * d.Ho * d.Wo, c.co, taps * c.ci
    return c.n * c.h * c.w, c.ci, taps * c.co


def class_taps(p, pad, dil, s, k):
    """taps of one axis that reach the input pixels of parity p (igemm_route.h tap_axis)"""
    return [t for t in range(k) if (p + pad - t * dil) % s == 0]


def dgrad_classes(c, d):
    """(ph, pw, rows, taps) of every parity class of a strided data gradient, in launch order"""
    out = []
    for ph in range(c.stride):
        for pw in range(c.stride):
            hq, wq = len(range(ph, c.h, c.stride)), len(range(pw, c.w, c.stride))
            taps = len(class_taps(ph, d.pad, d.dil, c.stride, d.KH)) * len(class_taps(pw, d.pad, d.dil, c.stride, d.KW))
            out.append((ph, pw, c.n * hq * wq, taps))
    return out


def in_classes(c, d, op):
    return op == DGRAD and c.stride > 1 and is_fast(c, d, op)


def combines(rec):
    """the slabs of this launch are combined inside it (splitk_combine_ok, and the fast kernels only)"""
    return rec.splits > 1 and rec.kloop != 0 and rec.bm == 64 and rec.bn <= 80 and not NO_COMBINE


def claim_text(c, d, op, rec):
    """the coverage claim that a launch record (or the host query's) amounts to"""
    s = "%s %dx%d x%d" % (KNAMES.get(rec.kloop, "kloop %d" % rec.kloop), rec.bm, rec.bn, rec.splits)
    if rec.splits > 1:
        s += " launch" if combines(rec) else " reduce"
    if rec.in_affine:
        s += " aff"
    if in_classes(c, d, op):
        s += " classes"
    return s


def class_record(hip_lib, lib, c, rows, taps):
    """the record of one parity class's launch: its own plan, the K loop by pair_loop_ok's rule"""
    bm, bn, sp, ks = (ctypes.c_int32() for _ in range(4))
    assert hip_lib.gs_debug_query_plan(rows, c.ci, max(taps, 1) * c.co, 64, ctypes.byref(bm), ctypes.byref(bn),
                                       ctypes.byref(sp), ctypes.byref(ks)) == 0
    tiles = -(-rows // bm.value) * -(-c.ci // bn.value) * sp.value
    assert tiles < 2 * hip_lib.gs_debug_num_cu(), "the class would pass the bf16x3 gate: pick another shape"
    pairs = ks.value >= 16 and tiles <= 3 * hip_lib.gs_debug_num_cu()
    return lib.DebugLaunch(lib.OP_DGRAD, lib.KLOOP_FP32_PAIRS if pairs else lib.KLOOP_FP32, bm.value, bn.value,
                           sp.value, ks.value, 0, 0)


def check_claim(hip_lib, lib, c, d, op, q, rec=None):
    """the host query `q` (and, after a launch, the record `rec`) against the case's coverage claim"""
    m, n, k = gemm_dims(c, d, op)
    classes = in_classes(c, d, op)
    for r in (q, rec):
        if r is None:
            continue
        assert r.op == (lib.OP_FORWARD if op == FWD else lib.OP_DGRAD)
        assert r.kloop in KNAMES or PLAN_ENV, "kloop %d: the stem, streaming, bf16x3 and f16 paths are not this file's" % r.kloop
        if op == FWD and not is_vector(c):      # (the stem kernel reports 128-row tiles under GEN)
            assert r.bm == 64 or PLAN_ENV, "the stem path is not this file's"
        assert r.in_affine == (1 if c.aff and op == FWD else 0) and r.bn_bwd_mode == 0
        assert (r.kloop == 0) == (not is_fast(c, d, op))
    if not classes:
        nk = -(-k // BK)
        assert q.splits >= 1 and q.splits * q.ksteps_per_split >= nk > (q.splits - 1) * q.ksteps_per_split
        if rec is not None:
            assert bytes(q) == bytes(rec), "the host query and the launch disagree"
    elif not PLAN_ENV:
        # the query describes class (0, 0), the record the last class that has taps and pixels
        cls = dgrad_classes(c, d)
        assert bytes(q) == bytes(class_record(hip_lib, lib, c, cls[0][2], cls[0][3]))
        if rec is not None:
            last = [x for x in cls if x[2] and x[3]][-1]
            assert bytes(rec) == bytes(class_record(hip_lib, lib, c, last[2], last[3])), "the last class's launch"
    if c.force:
        assert (q.bm, q.bn) == c.force[:2]
    if PLAN_ENV or NO_FAST or NO_COMBINE:
        return
    assert claim_text(c, d, op, q) == c.claim(op)


def exact_bound(c, d, op):
    """largest |value| the exact leg can reach: |x|, |w|, |dy| <= 3 (in_affine: the activation <= 11),
    plus bias and addend, or the accumulate base"""
    _, _, k = gemm_dims(c, d, op)
    return k * 3 * (11 if c.aff and op == FWD else 3) + (6 if op == FWD else 3)


# ------------------------------------------------------------------------------------------
# data and references (CPU; one set per shape and leg, shared by every case and op of that shape)
# ------------------------------------------------------------------------------------------
class Data(NamedTuple):
    x: torch.Tensor                  # [n, h, w, ci]
    w: torch.Tensor                  # [kh, kw, ci, co]
    bias: torch.Tensor               # [co]
    addend: torch.Tensor             # [n, ho, wo, co]
    coeffs: torch.Tensor             # [scale | beta | mean | invstd] x ci
    dy: torch.Tensor                 # [n, ho, wo, co]
    base: torch.Tensor               # [n, h, w, ci]: what the data gradient accumulates onto


def data_key(c):
    return c._replace(ci_max=None, co_ld=None, ldx=None, ldy=None, ld_add=None, nchw=False, nan_w=False,
                      force=None, fwd=None, dgr=None, bias=False, addend=False, aff=False)


@functools.lru_cache(maxsize=4)
def make_data(key, exact):
    from gaia_seg_amd.hip import lib
    c, d = key, make_desc(lib, key)
    gen = torch.Generator().manual_seed(31 if exact else 32)
    shapes = [(c.n, c.h, c.w, c.ci), (d.KH, d.KW, c.ci, c.co), (c.co,), (c.n, d.Ho, d.Wo, c.co),
              (c.n, d.Ho, d.Wo, c.co), (c.n, c.h, c.w, c.ci)]
    if exact:
        x, w, bias, addend, dy, base = (small_ints(gen, *s) for s in shapes)
        # integer mean and beta, scale in {0.5, 1, 2}: the activation is a multiple of 0.5 below 12;
        # beta - mean * scale > 0 on most channels, so a padded tap that went through the BatchNorm
        # would not be zero
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.ci,), generator=gen)]
        beta = torch.randint(1, 4, (c.ci,), generator=gen).float()
        mean = torch.randint(-1, 2, (c.ci,), generator=gen).float()
    else:
        x, w, bias, addend, dy, base = (torch.randn(*s, generator=gen) for s in shapes)
        scale, beta, mean = (torch.randn(c.ci, generator=gen) for _ in range(3))
    invstd = torch.rand(c.ci, generator=gen) + 0.5              # not read by the loaders
    return Data(x, w, bias, addend, torch.cat([scale, beta, mean, invstd]), dy, base)


def _logical_weight(t):
    return t.w.double().permute(3, 2, 0, 1)


@functools.lru_cache(maxsize=8)
def ref_forward(key, exact, bias, addend, aff):
    """float64 forward on the CPU as [n, ho, wo, co]"""
    from gaia_seg_amd.hip import lib
    c, d, t = key, make_desc(lib, key), make_data(key, exact)
    a = t.x.double()
    if aff:
        scale, beta, mean = (t.coeffs[i * c.ci:(i + 1) * c.ci].double() for i in range(3))
        a = F.relu((a - mean) * scale + beta)                  # zero padding applies to the activation
    y = F.conv2d(a.permute(0, 3, 1, 2), _logical_weight(t), t.bias.double() if bias else None, c.stride, d.pad,
                 c.dil).permute(0, 2, 3, 1)
    return (y + t.addend.double() if addend else y).contiguous()


@functools.lru_cache(maxsize=4)
def ref_dgrad(key, exact):
    """float64 input gradient on the CPU as [n, h, w, ci]"""
    from gaia_seg_amd.hip import lib
    c, d, t = key, make_desc(lib, key), make_data(key, exact)
    xz = torch.zeros(c.n, c.ci, c.h, c.w, dtype=torch.float64, requires_grad=True)
    F.conv2d(xz, _logical_weight(t), None, c.stride, d.pad, c.dil).backward(t.dy.double().permute(0, 3, 1, 2))
    return xz.grad.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------
# the launch helper
# ------------------------------------------------------------------------------------------
def _padded(t, pitch):
    """[..., c] at row pitch `pitch`, NaN in the columns past c"""
    out = torch.full(t.shape[:-1] + (pitch,), float("nan"))
    out[..., :t.shape[-1]] = t
    return out.to(DEV)


def run_case(hip_lib, lib, c, op, t, accumulate=0):
    """One synchronised launch under the rules of the module docstring: (active part of the output on
    the CPU, launch record).  Checks everything around the active part, the workspace and the claim."""
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    d = make_desc(lib, c)
    ldx, ldy = c.ldx or c.ci, c.ldy or c.co
    wg = torch.full((d.KH, d.KW, d.Ci_max, d.Co_ld), float("nan") if c.nan_w else POISON)
    wg[:, :, :c.ci, :c.co] = t.w
    wg = wg.to(DEV)
    rows_y, rows_x = c.n * d.Ho * d.Wo, c.n * c.h * c.w
    if op == FWD:
        xg = t.x.permute(0, 3, 1, 2).contiguous().to(DEV) if c.nchw else _padded(t.x, ldx)
        bias = t.bias.to(DEV) if c.bias else None
        addend = _padded(t.addend, d.ld_add) if c.addend else None
        coeffs = t.coeffs.to(DEV) if c.aff else None
        if c.aff:
            d.in_affine = coeffs.data_ptr()
            assert hip_lib.gs_conv2d_in_affine_supported(ctypes.byref(d)) == 1, "pick another shape"
        rows, width, pitch = rows_y, c.co, ldy
        out = torch.full((rows + GUARD_ROWS, pitch), SENTINEL, device=DEV)
    else:
        dyg = _padded(t.dy, ldy)
        rows, width, pitch = rows_x, c.ci, ldx
        out = torch.full((rows + GUARD_ROWS, pitch), SENTINEL)
        if accumulate:
            out[:rows, :width] = t.base.reshape(rows, width)
        out = out.to(DEV)
    q, rec = lib.DebugLaunch(), lib.DebugLaunch()
    with forced_plan(hip_lib, c):
        need = hip_lib.gs_conv2d_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=DEV)     # exactly `need` bytes of NaN, then the guard
        ws[:need] = 0xFF
        ws[need:] = GUARD_BYTE
        hip_lib.gs_debug_splitk_combined(1)
        if op == FWD:
            rc = hip_lib.gs_conv2d_forward(ctypes.byref(d), xg.data_ptr(), wg.data_ptr(),
                                           bias.data_ptr() if c.bias else None, addend.data_ptr() if c.addend else None,
                                           out.data_ptr(), ws.data_ptr(), need, current_stream_ptr())
        else:
            rc = hip_lib.gs_conv2d_dgrad(ctypes.byref(d), dyg.data_ptr(), wg.data_ptr(), out.data_ptr(), accumulate,
                                         ws.data_ptr(), need, current_stream_ptr())
        lib.check(rc, op)
        assert hip_lib.gs_debug_last_conv_launch(ctypes.byref(rec)) == 0
        assert hip_lib.gs_debug_query_conv_launch(ctypes.byref(d), lib.OP_FORWARD if op == FWD else lib.OP_DGRAD,
                                                  ctypes.byref(q)) == 0
        combined = hip_lib.gs_debug_splitk_combined(1)
        check_claim(hip_lib, lib, c, d, op, q, rec)
    torch.cuda.synchronize()
    classes = in_classes(c, d, op)
    if not classes:
        assert (combined > 0) == combines(rec), "in-launch combine: %d launches, claimed %s" % (combined, combines(rec))
        m, n, _ = gemm_dims(c, d, op)
        own = rec.splits * m * n * 4 if rec.splits > 1 else 0
        assert own <= need
        assert bool((ws[own:need] == 0xFF).all()), "a store behind this op's own slabs"
    assert bool((ws[need:] == GUARD_BYTE).all()), "the slabs overran the workspace"
    out = out.cpu()
    outside = torch.ones_like(out, dtype=torch.bool)
    outside[:rows, :width] = False
    assert bool((out[outside] == SENTINEL).all()), "%d stores outside [rows, :%d]" % (
        int((out[outside] != SENTINEL).sum()), width)
    active = out[:rows, :width].contiguous()
    assert bool(torch.isfinite(active).all()), "%d non-finite outputs: an unwritten slab cell or a pad column was read" % (
        int((~torch.isfinite(active)).sum()))
    shape = (c.n, d.Ho, d.Wo, c.co) if op == FWD else (c.n, c.h, c.w, c.ci)
    return active.view(shape), rec


def _assert_exact(got, want, what):
    diff = got.double() != want
    assert not bool(diff.any()), "%s: %d of %d elements differ, largest by %g, first at %s" % (
        what, int(diff.sum()), want.numel(), float((got.double() - want).abs().max()),
        tuple(int(i) for i in diff.nonzero()[0]))


def check_both_legs(hip_lib, c, op):
    from gaia_seg_amd.hip import lib
    key, d = data_key(c), make_desc(lib, c)
    ref = (lambda exact: ref_forward(key, exact, c.bias, c.addend, c.aff)) if op == FWD else (lambda exact: ref_dgrad(key, exact))
    # (a) exact
    t, want = make_data(key, True), ref(True)
    got, rec = run_case(hip_lib, lib, c, op, t)
    print("%s %s: %s, %d steps per split, max |want| %g" % (op, c.id(), claim_text(c, d, op, rec),
                                                           rec.ksteps_per_split, float(want.abs().max())))
    assert float(want.abs().max()) < EXACT_BOUND and exact_bound(c, d, op) < EXACT_BOUND
    _assert_exact(got, want, "exact leg")
    if op == DGRAD:
        if c.stride > 1:      # pixels no tap reaches: exactly zero under `=`
            for ph in range(c.stride):
                for pw in range(c.stride):
                    if not class_taps(ph, d.pad, d.dil, c.stride, d.KH) or not class_taps(pw, d.pad, d.dil, c.stride, d.KW):
                        assert not bool(got[:, ph::c.stride, pw::c.stride].any()), "tapless class (%d, %d)" % (ph, pw)
        acc, _ = run_case(hip_lib, lib, c, op, t, accumulate=1)
        assert float((want + t.base.double()).abs().max()) < EXACT_BOUND
        _assert_exact(acc, want + t.base.double(), "exact leg, accumulate")
    # (b) random, twice
    t, want = make_data(key, False), ref(False)
    first, _ = run_case(hip_lib, lib, c, op, t)
    second, _ = run_case(hip_lib, lib, c, op, t)
    err = rel_err(first, want)
    print("%s %s: random leg rel_err %.3g" % (op, c.id(), err))
    assert err < TOL
    assert torch.equal(first, second), "two runs of the same input differ"
    if op == DGRAD:
        acc, _ = run_case(hip_lib, lib, c, op, t, accumulate=1)
        err = rel_err(acc, want + t.base.double())
        print("%s %s: random leg, accumulate rel_err %.3g" % (op, c.id(), err))
        assert err < TOL


@pytest.mark.parametrize("case,op", PARAMS, ids=param_id)
def test_conv_rows(hip_lib, case, op):
    if case.aff and NO_FAST:
        pytest.skip("in_affine needs the fast kernels (GS_NO_FAST is set)")
    check_both_legs(hip_lib, case, op)
