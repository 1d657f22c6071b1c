"""The C-ABI harness the attention GPU tests share (test_attention_gpu.py, test_attention_f16_gpu.py,
test_beit_ops_gpu.py) and tests/golden/make_attention_parent_bits.py: the sentinel / NaN-padding /
guarded-workspace protocol described in test_attention_gpu.py, on the fp32 entries (``sfx`` "") or the
fp16-operand ones (``sfx`` "_f16")."""
import ctypes
import hashlib

import torch

import util_vit as U

DEV = "cuda"
SENTINEL = 7.0
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
NAN = float("nan")
GS_E_BADARG, GS_E_ALIGN, GS_E_WORKSPACE, GS_E_NULL = -1, -2, -3, -4
NAMES = ("O", "lse", "dQ", "dK", "dV", "dQ+", "dK+", "dV+")

# (name, B, Wh, Ww, heads, sliced operands + wide ldo + ld_table 4?, only the three cls rows non-zero?)
RELPOS_CASES = [
    ("2x3", 2, 2, 3, 1, False, False),
    ("5x7-crosses-a-key-tile", 1, 5, 7, 2, False, False),
    ("5x7-cls-rows-only", 1, 5, 7, 2, False, True),
    ("11x12-sliced-crosses-a-workgroup", 2, 11, 12, 3, True, False),
    ("12x11-transposed-window", 1, 12, 11, 3, False, False),
]


def make_table(wh, ww, heads, cls_only, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((2 * wh - 1) * (2 * ww - 1) + 3, heads, generator=g) * 2.0
    if cls_only:
        t[:-3] = 0
    return t


def stream():
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    return current_stream_ptr()


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
        assert bool((self.buf[self.need:] == GUARD_BYTE).all()), "the workspace was overrun"


def padded(t, ld, fill, c0=0):
    """t [..., c] inside a [..., ld] buffer filled with ``fill``, at column c0"""
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
    assert bool(torch.isfinite(got).all()), "%s: NaN -- a pad column, an inactive head or unwritten scratch " \
                                            "was read" % what
    return got


def _operands(b, n, heads, sliced, q, k, v):
    """-> (pointers of Q, K, V, their pitch, the pitch of O, what keeps them alive).  ``sliced``: Q, K, V are
    column slices of one buffer of 4 heads' width per operand whose 4th head holds NaN, and O gets a pitch
    wider than needed."""
    c = 64 * heads
    if sliced:
        hw = 64 * 4
        qkv = torch.full((b, n, 3 * hw), NAN)
        for i, t in enumerate((q, k, v)):
            qkv[..., i * hw:i * hw + c] = t
        qkv = qkv.to(DEV)
        return [qkv.data_ptr() + 4 * i * hw for i in range(3)], 3 * hw, c + 24, [qkv]
    keep = [t.contiguous().to(DEV) for t in (q, k, v)]
    return [t.data_ptr() for t in keep], c, c, keep


def _lse_rows(lse, b, heads, n):
    lse_cpu = lse.cpu()
    assert bool((lse_cpu[b * heads * n:] == SENTINEL).all()), "lse: a store past [B][heads][N]"
    return lse_cpu[:b * heads * n].view(b, heads, n)


def run_attention(L, lib, b, n, heads, sliced, q, k, v, do, bases, sfx="", scale=U.SCALE):
    """forward, backward (overwrite), backward (accumulate onto the bases) -> (O, lse, dQ, dK, dV, dQ+, dK+,
    dV+) of the entries with suffix ``sfx``.  ``sliced``: Q, K, V (and dQ, dK, dV) are column slices of one
    buffer of 4 heads' width per operand -- the 4th head's columns hold NaN (inputs) / the sentinel (outputs)
    -- and O / dO have a pitch wider than needed."""
    fwd, bwd = getattr(L, "gs_attention_forward" + sfx), getattr(L, "gs_attention_backward" + sfx)
    ws_bytes = getattr(L, "gs_attention_workspace_bytes" + sfx)
    c, hw = 64 * heads, 64 * 4
    ptrs, ldq, ldo, keep = _operands(b, n, heads, sliced, q, k, v)
    d = lib.attention_desc(b, n, heads, scale, ldq=ldq, ldk=ldq, ldv=ldq, ldo=ldo)
    db, st = ctypes.byref(d), stream()
    o = torch.full((b, n, ldo), SENTINEL, device=DEV)
    lse = torch.full((b * heads * n + 8,), SENTINEL, device=DEV)
    lib.check(fwd(db, ptrs[0], ptrs[1], ptrs[2], o.data_ptr(), lse.data_ptr(), st), "fwd")
    o_got = active(o, 0, c, "O")
    lse_got = _lse_rows(lse, b, heads, n)
    dog = padded(do, ldo, NAN)
    outs = []
    for accumulate in (0, 1):
        if sliced:   # the three gradients as slices of one buffer, like the operands
            g = torch.full((b, n, 3 * hw), SENTINEL)
            if accumulate:
                for i, t in enumerate(bases):
                    g[..., i * hw:i * hw + c] = t
            g = g.to(DEV)
            gptrs = [g.data_ptr() + 4 * i * hw for i in range(3)]
            c0s = [0, hw, 2 * hw]
        else:
            gbufs = [(bases[i].contiguous().to(DEV) if accumulate else torch.full((b, n, c), SENTINEL, device=DEV))
                     for i in range(3)]
            gptrs = [t.data_ptr() for t in gbufs]
        ws = Workspace(ws_bytes(db))
        lib.check(bwd(db, ptrs[0], ptrs[1], ptrs[2], o.data_ptr(), lse.data_ptr(), dog.data_ptr(), gptrs[0],
                      gptrs[1], gptrs[2], accumulate, ws.ptr(), ws.need, st), "bwd")
        ws.check()
        if sliced:
            full = g.cpu()
            outside = torch.ones_like(full, dtype=torch.bool)
            for c0 in c0s:
                outside[..., c0:c0 + c] = False
            assert bool((full[outside] == SENTINEL).all()), "a gradient store outside the active columns"
            got = [full[..., c0:c0 + c].contiguous() for c0 in c0s]
        else:
            got = [t.cpu() for t in gbufs]
        for name, t in zip(("dQ", "dK", "dV"), got):
            assert bool(torch.isfinite(t).all()), "%s: NaN -- a pad column or unwritten scratch was read" % name
        outs += got
    del keep
    return (o_got, lse_got) + tuple(outs)


def run_relpos(L, lib, b, wh, ww, heads, sliced, q, k, v, table, sfx=""):
    """-> (O, lse) of gs_attention_relpos_forward + ``sfx``; ``table`` None runs gs_attention_forward + ``sfx``
    on the same operands.  ``sliced``: as for run_attention, and the table has a 4th column of NaN (ld_table
    4 for 3 heads)."""
    n, c = wh * ww + 1, 64 * heads
    ptrs, ldq, ldo, keep = _operands(b, n, heads, sliced, q, k, v)
    ldt = heads + 1 if sliced else heads
    d = lib.attention_desc(b, n, heads, U.SCALE, ldq=ldq, ldk=ldq, ldv=ldq, ldo=ldo)
    o = torch.full((b, n, ldo), SENTINEL, device=DEV)
    lse = torch.full((b * heads * n + 8,), SENTINEL, device=DEV)
    if table is None:
        lib.check(getattr(L, "gs_attention_forward" + sfx)(ctypes.byref(d), ptrs[0], ptrs[1], ptrs[2], o.data_ptr(),
                                                           lse.data_ptr(), stream()), "plain forward")
    else:
        tg = torch.full((table.shape[0], ldt), NAN)
        tg[:, :heads] = table
        tg = tg.to(DEV)
        lib.check(getattr(L, "gs_attention_relpos_forward" + sfx)(
            ctypes.byref(d), ptrs[0], ptrs[1], ptrs[2], tg.data_ptr(), ldt, wh, ww, o.data_ptr(), lse.data_ptr(),
            stream()), "relpos forward")
    o_got = active(o, 0, c, "O")
    lse_got = _lse_rows(lse, b, heads, n)
    assert bool(torch.isfinite(lse_got).all()), "lse: NaN"
    del keep
    return o_got, lse_got


# ---- bit-for-bit digests (tests/golden/attention_parent_bits.json) -----------------------------------------
PRECISIONS = {"fp32": "", "fp16": "_f16"}
ATTENTION_SEEDS = {"fp32": 5, "fp16": 1}   # the seeds of the two forward_backward tests
BITS_CASES = [("attention", c) for c in U.ATTENTION_CASES] + [("relpos", c) for c in RELPOS_CASES]


def sha256_f32(t):
    """SHA-256 of the little-endian fp32 bytes of a CPU tensor"""
    return hashlib.sha256(t.contiguous().numpy().astype("<f4").tobytes()).hexdigest()


def output_digests(L, lib, kind, case, precision):
    """{quantity: digest} of the active slices of one case's outputs: O, lse, dQ, dK, dV with accumulate 0 and
    (as dQ+, dK+, dV+) 1 for an entry of util_vit.ATTENTION_CASES, O and lse for one of RELPOS_CASES"""
    sfx = PRECISIONS[precision]
    if kind == "attention":
        _, b, n, heads, sliced, dominant = case
        q, k, v, do, bq, bk, bv = U.attention_inputs(b, n, heads, dominant, ATTENTION_SEEDS[precision])
        got = run_attention(L, lib, b, n, heads, sliced, q, k, v, do, (bq, bk, bv), sfx=sfx)
    else:
        _, b, wh, ww, heads, sliced, cls_only = case
        q, k, v = U.attention_inputs(b, wh * ww + 1, heads, False, 7)[:3]
        got = run_relpos(L, lib, b, wh, ww, heads, sliced, q, k, v, make_table(wh, ww, heads, cls_only, 11), sfx=sfx)
    return {nm: sha256_f32(t) for nm, t in zip(NAMES, got)}
