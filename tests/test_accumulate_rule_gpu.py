"""The one accumulate rule of the tape ops (ops._input_grad: the flag is "the target held something before
this call") on the GPU, where it changed what a kernel is asked: ops.attention and ops.attention_kv on
slices of one fresh buffer, and map_pad / map_crop / the residual hand-on on a slice, now WRITE (flag 0) where
they used to ACCUMULATE (flag 1) onto the zeros the owning buffer's gradient is allocated with.

Every case checks three things:
  * the tape's gradients are torch.equal to a direct C-ABI call of the same backward with accumulate = 1
    onto zero-filled targets of the same layout, which is what the ops asked for before (torch.equal, not a
    digest: 0 + (-0) is +0 and the two compare equal);
  * they are within the tolerance of the op's own GPU test of the project's float64 formula (TOL = 3e-5 of
    test_attention_gpu.py / test_attention_kv_gpu.py / test_window_attention_gpu.py; for the fp16 entries
    util_attention_f16.FACTOR times the error of the CPU witness, as test_attention_f16_gpu.py); the copies are
    exact;
  * two runs agree bit for bit.
ops.window_attention already followed the rule: its cases guard the body the three q / k / v ops now share.
The ``held`` cases give k a gradient before the call, as a second consumer would: the flag is 1 and the result
the sum."""
import contextlib
import ctypes

import pytest
import torch

from conftest import rel_err
import util_attention_f16 as W
import util_mit as M
import util_swin as S
import util_vit as U
from util_attention_gpu import DEV, stream

pytestmark = pytest.mark.gpu
TOL = 3e-5


def _maps(ts, shape):
    """[b, n, c] CPU tensors as contiguous [b, h, w, c] device maps"""
    return [t.view(*shape, t.shape[-1]).contiguous().to(DEV) for t in ts]


class _Case:
    """One q / k / v op at one shape: the inputs, the float64 reference and how to call the op and the library."""

    def __init__(self, op, b, q_hw, kv_hw, heads, seed, ws=0, shift=0, f16=False):
        self.op, self.b, self.q_hw, self.kv_hw, self.heads, self.f16 = op, b, q_hw, kv_hw, heads, f16
        self.ws, self.shift = ws, shift
        nq, nk = q_hw[0] * q_hw[1], kv_hw[0] * kv_hw[1]
        self.table = None
        if op == "attention":
            q, k, v, do, bq, bk, bv = U.attention_inputs(b, nq, heads, False, seed)
            ref = U.attention_ref(q, k, v, do, heads)
            if f16:
                self.witness = dict(zip(("O", "lse", "dQ", "dK", "dV"), W.witness(q, k, v, do, heads)))
        elif op == "attention_kv":
            q, k, v, do, bq, bk, bv = M.kv_inputs(b, nq, nk, heads, False, seed)
            ref = M.kv_ref(q, k, v, do, heads)
        else:
            q, k, v, do, (bq, bk, bv, _), table = S.wa_inputs(b, q_hw[0], q_hw[1], ws, heads, False, seed)
            # a max-size table of heads + 1 columns: the last one is idle
            self.table = torch.cat([table, torch.full((table.shape[0], 1), 0.25)], dim=1)
            ref = S.wa_ref(q, k, v, self.table, do, b, q_hw[0], q_hw[1], ws, shift, heads)
        self.c = q.shape[-1]
        self.q, = _maps([q], (b,) + q_hw)
        self.k, self.v = _maps([k, v], (b,) + kv_hw)
        self.do, = _maps([do], (b,) + q_hw)
        self.base_k, = _maps([bk], (b,) + kv_hw)
        self.ref = dict(zip(("O", "lse", "dQ", "dK", "dV", "dTable"), ref))
        self.ref_base_k = bk.double()

    # ---- layouts: q, k, v (and their gradients) as the slices the models use, or as separate activations ----
    def operands(self, sliced):
        """fresh device tensors holding q, k, v -> ([q, k, v] views, [the buffers that own them])"""
        if not sliced:
            own = [self.q.clone(), self.k.clone(), self.v.clone()]
            return own, own
        c = self.c
        if self.op == "attention_kv":           # q its own map, k and v two slices of the reduced map's buffer
            q, kv = self.q.clone(), torch.cat([self.k, self.v], dim=-1)
            return [q, kv[..., :c], kv[..., c:]], [q, kv]
        qkv = torch.cat([self.q, self.k, self.v], dim=-1)
        return [qkv[..., i * c:(i + 1) * c] for i in range(3)], [qkv]

    def desc(self, lib, ts, grads, ldo):
        ld = dict(zip(("ldq", "ldk", "ldv", "lddq", "lddk", "lddv"), [t.stride(2) for t in ts + grads]), ldo=ldo,
                  lddo=ldo)
        nq, nk = self.q_hw[0] * self.q_hw[1], self.kv_hw[0] * self.kv_hw[1]
        if self.op == "attention":
            return lib.attention_desc(self.b, nq, self.heads, U.SCALE, **ld)
        if self.op == "attention_kv":
            return lib.attention_kv_desc(self.b, nq, nk, self.heads, U.SCALE, **ld)
        return lib.window_attention_desc(self.b, self.q_hw[0], self.q_hw[1], self.ws, self.shift, self.heads,
                                         ld_table=self.table.shape[1], scale=S.SCALE, **ld)

    def direct(self, L, lib, sliced, held):
        """The library called directly: forward, then backward with accumulate = 1 onto zero-filled gradients of
        the tape's layout (k's holding the base where ``held``) -> {name: CPU tensor}"""
        ts, keep = self.operands(sliced)
        grads, gkeep = self.operands(sliced)
        for g in gkeep:
            g.zero_()
        if held:
            grads[1].copy_(self.base_k)
        o = torch.empty_like(self.do)
        d = self.desc(lib, ts, grads, o.stride(2))
        nq = self.q_hw[0] * self.q_hw[1]
        lse = torch.empty(self.b * self.heads * nq, dtype=torch.float32, device=DEV)
        stem = "gs_%s_%%s%s" % (self.op, "_f16" if self.f16 else "")
        tbl = gt = ()
        if self.table is not None:
            table, gtable = self.table.to(DEV), torch.zeros_like(self.table, device=DEV)
            tbl, gt = (table.data_ptr(),), (gtable.data_ptr(),)
        db, st = ctypes.byref(d), stream()
        lib.check(getattr(L, stem % "forward")(db, *(t.data_ptr() for t in ts), *tbl, o.data_ptr(), lse.data_ptr(),
                                               st), stem % "forward")
        need = getattr(L, stem % "workspace_bytes")(db)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        lib.check(getattr(L, stem % "backward")(db, *(t.data_ptr() for t in ts), *tbl, o.data_ptr(), lse.data_ptr(),
                                                self.do.data_ptr(), *(g.data_ptr() for g in grads), *gt, 1,
                                                ws.data_ptr(), need, st), stem % "backward")
        torch.cuda.synchronize()
        got = dict(O=o.cpu(), dQ=grads[0].cpu(), dK=grads[1].cpu(), dV=grads[2].cpu())
        if self.table is not None:
            got["dTable"] = gtable.cpu()
        del keep
        return got

    def tape(self, L, sliced, held):
        """The op on the tape -> {name: CPU tensor}; the backward entry is asked with the flag ``held``"""
        from gaia_seg_amd.hip import ops
        from gaia_seg_amd.hip.runtime import Act, Tape
        _, own = self.operands(sliced)
        own = [Act(t) for t in own]
        c = self.c
        if not sliced:
            q, k, v = own
        elif self.op == "attention_kv":
            q, k, v = own[0], own[1].slice(0, c), own[1].slice(c, 2 * c)
        else:
            q, k, v = (own[0].slice(i * c, (i + 1) * c) for i in range(3))
        if held:
            k.new_grad().copy_(self.base_k)
        tape = Tape()
        tp = None
        entry = "gs_%s_backward%s" % (self.op, "_f16" if self.f16 else "")
        real, flags = getattr(L, entry), []

        def spy(*a):
            flags.append(a[-4])     # (..., accumulate, workspace, its size, stream)
            return real(*a)
        setattr(L, entry, spy)
        try:
            if self.op == "attention":
                out = ops.attention(tape, q, k, v, self.heads, U.SCALE, f16=self.f16)
            elif self.op == "attention_kv":
                out = ops.attention_kv(tape, q, k, v, self.heads, U.SCALE)
            else:
                tp = torch.nn.Parameter(self.table.to(DEV))
                out = ops.window_attention(tape, q, k, v, tp, self.heads, self.ws, self.shift, S.SCALE)
            out.g = self.do.clone()
            tape.backward()
        finally:
            setattr(L, entry, real)
        torch.cuda.synchronize()
        assert flags == [1 if held else 0], flags
        got = dict(O=out.t.cpu(), dQ=q.g.cpu(), dK=k.g.cpu(), dV=v.g.cpu())
        if tp is not None:
            got["dTable"] = tp.grad.cpu()
        return got

    def check(self, hip_lib, sliced, held):
        from gaia_seg_amd.hip import lib
        first, second = self.tape(hip_lib, sliced, held), self.tape(hip_lib, sliced, held)
        direct = self.direct(hip_lib, lib, sliced, held)
        for name, t in first.items():
            assert torch.equal(t, second[name]), "%s differs between two runs" % name
            assert torch.equal(t, direct[name]), "%s differs from accumulate = 1 onto zeros" % name
        for name, t in first.items():
            want = self.ref[name]
            got = t.reshape(self.b, -1, t.shape[-1]) if name != "dTable" else t[:, :self.heads]
            if held and name == "dK":
                want = want + self.ref_base_k
            err = rel_err(got, want)
            bound = W.FACTOR * rel_err(self.witness[name], self.ref[name]) if self.f16 else TOL
            print("%s %s: rel_err %.3e (bound %.3e)" % (self.op, name, err, bound))
            assert err <= bound, "%s: rel_err %.3g > %.3g" % (name, err, bound)
        if "dTable" in first:
            assert not bool(first["dTable"][:, self.heads:].any()), "the idle table column got a gradient"


@pytest.mark.parametrize("n,f16", [(33, False), (129, False), (33, True)], ids=["N33", "N129", "N33-f16"])
def test_attention_on_slices_of_one_fresh_buffer(hip_lib, n, f16):
    """past one 32-key tile and past one 128-query tile; q, k, v three slices of one buffer: the flag is 0"""
    from gaia_seg_amd.hip import ops
    with ops.train_precision("fp16") if f16 else contextlib.nullcontext():
        _Case("attention", 2, (1, n), (1, n), 2, seed=21, f16=f16).check(hip_lib, sliced=True, held=False)


def test_attention_kv_on_slices_of_one_fresh_buffer(hip_lib):
    _Case("attention_kv", 2, (5, 7), (2, 3), 1, seed=22).check(hip_lib, sliced=True, held=False)


@pytest.mark.parametrize("shift", [0, 2])
def test_window_attention_on_slices_of_one_fresh_buffer(hip_lib, shift):
    _Case("window_attention", 1, (8, 8), (8, 8), 2, seed=23, ws=4, shift=shift).check(hip_lib, sliced=True, held=False)


@pytest.mark.parametrize("op", ["attention", "attention_kv", "window_attention"])
def test_a_held_gradient_is_added_to(hip_lib, op):
    """k's gradient exists before the call: flag 1, the fresh dQ and dV start from zero, dK is the sum"""
    case = {"attention": lambda: _Case("attention", 2, (1, 33), (1, 33), 2, seed=24),
            "attention_kv": lambda: _Case("attention_kv", 2, (5, 7), (2, 3), 1, seed=25),
            "window_attention": lambda: _Case("window_attention", 1, (8, 8), (8, 8), 2, seed=26, ws=4, shift=2)}[op]()
    case.check(hip_lib, sliced=False, held=True)


# ---- the single-input ops whose flag changed for a slice: map_pad, map_crop, the residual hand-on ----------------
def _slice_case(run, direct, x_hw, dy_hw, want):
    """``run(tape, x) -> out`` on x = the leading 8 of 16 columns of a fresh buffer, under an upstream gradient
    dy; ``direct(dy, dx)``: the library's backward entry with accumulate = 1; ``want(dy)``: the exact result"""
    from gaia_seg_amd.hip.runtime import Act, Tape
    g = torch.Generator().manual_seed(27)
    x = torch.randn(1, *x_hw, 16, generator=g).to(DEV)
    dy = torch.randn(1, *dy_hw, 8, generator=g).to(DEV)

    def once():
        owner = Act(x.clone())
        a = owner.slice(0, 8)
        tape = Tape()
        out = run(tape, a)
        assert tuple(out.t.shape) == tuple(dy.shape)
        out.g = dy.clone()
        tape.backward()
        torch.cuda.synchronize()
        return owner.g.cpu()
    first, second = once(), once()
    old = torch.zeros_like(x)
    direct(dy, old[..., :8])
    torch.cuda.synchronize()
    assert torch.equal(first, second), "two runs differ"
    assert torch.equal(first, old.cpu()), "differs from accumulate = 1 onto zeros"
    assert torch.equal(first[..., :8], want(dy.cpu())) and not bool(first[..., 8:].any())


def test_map_pad_and_crop_write_a_fresh_slice(hip_lib):
    from gaia_seg_amd.hip import lib, ops
    L = hip_lib

    def crop_into(dy, dx):      # the backward of map_pad: [1, 8, 8, 8] -> the leading 5 x 6
        lib.check(L.gs_map_crop(dy.data_ptr(), dy.stride(2), dx.data_ptr(), dx.stride(2), 1, 5, 6, 8, 8, 8, 1, stream()),
                  "gs_map_crop")

    def pad_into(dy, dx):       # the backward of map_crop: [1, 5, 6, 8] -> zero-padded to 8 x 8
        lib.check(L.gs_map_pad(dy.data_ptr(), dy.stride(2), dx.data_ptr(), dx.stride(2), 1, 5, 6, 8, 8, 8, 1, stream()),
                  "gs_map_pad")
    _slice_case(lambda tape, a: ops.map_pad(tape, a, 8, 8), crop_into, (5, 6), (8, 8), lambda dy: dy[:, :5, :6])
    _slice_case(lambda tape, a: ops.map_crop(tape, a, 5, 6), pad_into, (8, 8), (5, 6),
                lambda dy: torch.nn.functional.pad(dy, (0, 0, 0, 2, 0, 3)))


def test_residual_hand_on_writes_a_fresh_slice(hip_lib):
    """layer_scale_add(gamma=None): the identity, a slice, gets the output's gradient by one copy"""
    from gaia_seg_amd.hip import lib, ops
    from gaia_seg_amd.hip.runtime import Act
    L = hip_lib
    z = torch.randn(1, 5, 6, 8, generator=torch.Generator().manual_seed(28)).to(DEV)

    def copy_into(dy, dx):
        lib.check(L.gs_copy2d(dy.data_ptr(), dy.stride(2), dx.data_ptr(), dx.stride(2), 30, 8, 1.0, 1, stream()),
                  "gs_copy2d")
    _slice_case(lambda tape, a: ops.layer_scale_add(tape, a, Act(z.clone()), None), copy_into, (5, 6), (5, 6),
                lambda dy: dy)
