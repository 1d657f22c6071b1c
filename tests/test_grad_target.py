"""ops._grad_target: where a backward kernel writes the gradient of an input, and with which flag
(no GPU needed: the helper only allocates and looks at layouts).

The flag follows one rule (``ops._input_grad``): the target held something before this call.  The
second half of this file pins it for the ops that pass the flag on, with the library entries replaced
by a recording stub as in tests/host_dry_run.py.

The frozen-slice case is the one the helper exists for: layernorm's kernel addresses dx with the
descriptor's ldx, and the ops used to hand it ``torch.empty_like`` of the view, a dense buffer of
pitch C -- rows * ld floats written into rows * C."""
import pytest
import torch

from gaia_seg_amd.hip import ops
from gaia_seg_amd.hip.runtime import Act, Tape


def test_frozen_slice_gets_scratch_of_its_own_pitch():
    buf = torch.zeros(1, 2, 3, 16)
    x = Act(buf[..., :8], requires_grad=False)
    assert torch.empty_like(x.t).stride(2) == 8          # what the ops used to allocate
    dx, acc = ops._grad_target(x)
    assert acc == 0
    assert dx.shape == x.t.shape and dx.stride() == x.t.stride() and dx.stride(2) == 16
    assert x.g is None                                    # nothing is kept for an input that needs none
    assert dx.data_ptr() != x.t.data_ptr()
    dx2, acc2 = ops._grad_target(x, "the map")            # (no consumer count for scratch)
    assert acc2 == 0 and dx2.stride(2) == 16


def test_root_gradient_is_fresh_then_accumulates():
    x = Act(torch.zeros(1, 2, 3, 8))
    g, acc = ops._grad_target(x)
    assert acc == 0 and g is x.g and g.stride() == x.t.stride()
    g2, acc2 = ops._grad_target(x)
    assert acc2 == 1 and g2.data_ptr() == g.data_ptr()


def test_sole_consumer_raises_on_a_held_gradient():
    x = Act(torch.zeros(1, 2, 3, 8))
    g, acc = ops._grad_target(x, "the map")
    assert acc == 0 and g is x.g
    with pytest.raises(RuntimeError, match="the map has more than one consumer"):
        ops._grad_target(x, "the map")


def test_slices_share_the_zeroed_gradient_of_their_buffer():
    parent = Act(torch.ones(1, 2, 3, 16))
    a, b = parent.slice(0, 8), parent.slice(8, 16)
    ga, acc_a = ops._grad_target(a)
    assert acc_a == 0 and ga.stride(2) == 16 and ga.shape == a.t.shape
    assert float(parent.g.abs().sum()) == 0.0             # allocated zeroed: b may accumulate
    gb, acc_b = ops._grad_target(b)
    assert acc_b == 1 and gb.data_ptr() == parent.g.data_ptr() + 8 * 4


def test_padded_pitch_is_kept():
    x = Act.empty(1, 2, 3, 19, torch.device("cpu"), requires_grad=False)   # 19 classes in 20 floats
    dx, acc = ops._grad_target(x)
    assert (acc, dx.stride(2), tuple(dx.shape)) == (0, 20, (1, 2, 3, 19))


# ---- the one accumulate rule, at the ops that pass the flag to a kernel -----------------------------------

class _Recorder:
    """Every library entry is a no-op that records (entry, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return 1024 if name.endswith("_bytes") else 0
        return f

    def flag(self, entry, index):
        """Argument ``index`` of the one recorded call of ``entry``."""
        hits = [a for n, a in self.calls if n == entry]
        assert len(hits) == 1, (entry, [n for n, _ in self.calls])
        return hits[0][index]


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(ops, "_L", lambda: r)
    monkeypatch.setattr(ops, "current_stream_ptr", lambda: 0)
    return r


def _backward_of(tape, out):
    """Run the closure the op recorded, under an upstream gradient of ones; the forward's calls are dropped."""
    out.g = torch.ones_like(out.t)
    (closure,) = tape.ops
    closure()


def _only_the_owner_holds_storage(owner, *slices):
    assert owner._g is not None and all(s._g is None for s in slices)
    for s in slices:
        assert s.g.data_ptr() == owner._g.data_ptr() + 4 * s.c0 and s.g.stride(2) == owner._g.stride(2)


def test_input_grad_flag_is_held_before_the_call():
    x = Act(torch.zeros(1, 2, 3, 8))
    assert ops._input_grad(x) == 0 and x.g is not None     # root: fresh
    assert ops._input_grad(x) == 1                         # root: held
    owner = Act(torch.ones(1, 2, 3, 16))
    a, b = owner.slice(0, 8), owner.slice(8, 16)
    assert ops._input_grad(a) == 0                         # a slice of a fresh buffer
    assert float(owner.g.abs().sum()) == 0.0               # ... whose gradient is all zeros
    _only_the_owner_holds_storage(owner, a, b)
    assert ops._input_grad(b) == 1                         # the sibling allocated the owner's gradient


def _pad(rec, x):
    tape = Tape()
    _backward_of(tape, ops.map_pad(tape, x, 4, 4))


def _crop(rec, x):
    tape = Tape()
    _backward_of(tape, ops.map_crop(tape, x, 1, 2))


def _residual(rec, x):
    ops._pass_residual_grad(rec, x, torch.ones(1, 2, 3, 8), x.rows, x.C, 0)


# (what runs, the entry that writes x's gradient, index of its accumulate argument)
@pytest.mark.parametrize("run,entry,index", [(_pad, "gs_map_crop", 10), (_crop, "gs_map_pad", 10),
                                             (_residual, "gs_copy2d", 7)],
                         ids=["map_pad", "map_crop", "pass_residual_grad"])
def test_single_input_ops_pass_the_rule_for_a_slice(rec, run, entry, index):
    for held, want in ((False, 0), (True, 1)):
        owner = Act(torch.zeros(1, 2, 3, 16))
        x, sibling = owner.slice(0, 8), owner.slice(8, 16)
        if held:
            ops._input_grad(sibling)
        run(rec, x)
        name, args = rec.calls[-1]                         # (the forward's call of an op comes before)
        assert name == entry and args[index] == want, (held, name, args)
        _only_the_owner_holds_storage(owner, x, sibling)
        assert float(owner.g.abs().sum()) == 0.0           # (allocated zeroed; the stub wrote nothing)


def _qkv_ops():
    def attention(tape, q, k, v, table):
        return ops.attention(tape, q, k, v, 1, 0.125)

    def attention_kv(tape, q, k, v, table):
        return ops.attention_kv(tape, q, k, v, 1, 0.125)

    def window_attention(tape, q, k, v, table):
        return ops.window_attention(tape, q, k, v, table, 2, 2, 0, 0.125)

    return [(attention, "gs_attention_backward", 10, (1, 1, 6, 64)),
            (attention_kv, "gs_attention_kv_backward", 10, (1, 2, 3, 64)),
            (window_attention, "gs_window_attention_backward", 12, (1, 2, 4, 64))]


@pytest.mark.parametrize("op,entry,index,shape", _qkv_ops(), ids=["attention", "attention_kv", "window_attention"])
def test_qkv_slices_of_one_fresh_buffer_are_written(rec, op, entry, index, shape):
    n, h, w, c = shape
    owner = Act(torch.zeros(n, h, w, 3 * c))
    q, k, v = (owner.slice(i * c, (i + 1) * c) for i in range(3))
    table = torch.nn.Parameter(torch.zeros(9, 3))
    tape = Tape()
    out = op(tape, q, k, v, table)
    _backward_of(tape, out)
    assert rec.flag(entry, index) == 0
    _only_the_owner_holds_storage(owner, q, k, v)


@pytest.mark.parametrize("op,entry,index,shape", _qkv_ops(), ids=["attention", "attention_kv", "window_attention"])
def test_qkv_with_one_gradient_held_accumulate_onto_zeroed_fresh_ones(rec, op, entry, index, shape):
    q, k, v = (Act(torch.zeros(*shape)) for _ in range(3))
    k.new_grad().fill_(3.0)
    table = torch.nn.Parameter(torch.zeros(9, 3))
    tape = Tape()
    out = op(tape, q, k, v, table)
    _backward_of(tape, out)
    assert rec.flag(entry, index) == 1
    assert float(q.g.abs().sum()) == 0.0 and float(v.g.abs().sum()) == 0.0   # (torch.empty otherwise)
    assert bool((k.g == 3.0).all())
