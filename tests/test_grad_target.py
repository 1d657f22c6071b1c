"""ops._grad_target: where a backward kernel writes the gradient of an input, and with which flag
(no GPU needed: the helper only allocates and looks at layouts).

The frozen-slice case is the one the helper exists for: layernorm's kernel addresses dx with the
descriptor's ldx, and the ops used to hand it ``torch.empty_like`` of the view, a dense buffer of
pitch C -- rows * ld floats written into rows * C."""
import pytest
import torch

from gaia_seg_amd.hip import ops
from gaia_seg_amd.hip.runtime import Act


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
