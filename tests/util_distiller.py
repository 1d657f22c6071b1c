"""Helpers of the DynamicDistiller tests: a torch restatement of the two distillation losses
(gaiaseg/models/segmentors/dynamic_distiller.py:309-356,397-403; tests/test_distiller.py holds it
against the values the reference's own methods produced, tests/golden/ref_distiller.npz), the
fixture's case tables and the seeded inputs that are regenerated instead of stored."""
import os

import numpy as np
import torch
import torch.nn.functional as F

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_distiller.npz")

# tag: (N, Cs, Ct, H, W, T, weight, numpy seed of the window draw, non-contiguous student?)
PAIRWISE_CASES = {
    "a": (2, 24, 40, 6, 10, 1.0, 1.0, 11, False),
    "b": (2, 96, 64, 7, 9, 2.0, 0.5, 12, False),
    "c": (2, 20, 36, 9, 5, 1.0, 1.0, 13, True),
    "zero": (2, 16, 12, 8, 6, 1.0, 1.0, 14, False),
}
PRODUCTION = (1, 2560, 2560, 16, 32, 1.0, 1.0, 15)   # regenerated from PRODUCTION_SEED, not stored
PRODUCTION_SEED = 20251

# tag: (N, Cls, (hs, ws), (ht, wt), (H, W), align_corners, T, weight)
DISTILL_CASES = {
    "a": (2, 19, (5, 7), (9, 13), (33, 49), False, 1.0, 1.0),
    "b": (2, 5, (5, 7), (9, 13), (33, 49), True, 2.5, 0.7),
    "c": (2, 19, (8, 8), (4, 6), (30, 41), False, 2.5, 1.0),
    "d": (2, 5, (8, 8), (4, 6), (30, 41), True, 1.0, 1.0),
    "e": (2, 19, (5, 7), (5, 7), (33, 49), False, 2.5, 1.0),
    "f": (2, 5, (6, 9), (6, 9), (24, 36), True, 1.0, 0.7),
}


def window_of(H, W, seed):
    """The reference's draw (dynamic_distiller.py:323-328) for numpy's global state seeded with
    ``seed``: (y0, y1, x0, x1, step_h, step_w) of the one column its slice selects."""
    rs = np.random.RandomState(seed)
    step_h, step_w = int(0.5 * H), int(0.5 * W)
    choice_h = rs.uniform(0, 0.5)
    choice_w = rs.uniform(0, 0.5)
    start_h, start_w = int(choice_h * H), int(choice_w * W)
    return (start_h, start_h + step_h, start_w + step_w, start_w + step_w + 1, step_h, step_w)


def ref_distill_loss(student, teacher, out_hw, T, weight, align_corners):
    """forward_train :397-403 + prepare_distill_feature :269-273 + distill_loss :352-356."""
    size = (int(out_hw[0]), int(out_hw[1]))
    s = F.interpolate(student, size=size, mode="bilinear", align_corners=align_corners)
    t = F.interpolate(teacher, size=size, mode="bilinear", align_corners=align_corners)
    n, _, h, w = s.shape
    return weight * -torch.sum(F.softmax(t / T, dim=1) * F.log_softmax(s / T, dim=1)) / (n * h * w)


def ref_pairwise_loss(student, teacher, window, T, weight):
    """pairwise_loss :320-339 with the window already drawn."""
    y0, y1, x0, _x1, step_h, step_w = window
    n = student.size(0)
    s = student[:, :, y0:y1, x0]
    t = teacher[:, :, y0:y1, x0]
    s = F.normalize(s, dim=1)
    t = F.normalize(t, dim=1)
    s = s.reshape(s.size(0), s.size(1), -1)
    t = t.reshape(t.size(0), t.size(1), -1)
    gs = torch.bmm(s.transpose(1, 2), s)
    gt = torch.bmm(t.transpose(1, 2), t)
    return weight * -torch.sum(F.softmax(gt / T, dim=1) * F.log_softmax(gs / T, dim=2)) / (n * step_h * step_w)


def embed_window(win, H, W, window, seed, noncontiguous=False):
    """A full [N, C, H, W] map, channels-last in memory, whose window column is ``win`` [N, C, P] and
    whose other pixels are seeded post-ReLU noise (they do not enter the loss).  ``noncontiguous``:
    the map is a channel slice of a wider channels-last buffer (pixel stride C + 12)."""
    n, c, p = win.shape
    y0, y1, x0 = window[0], window[1], window[2]
    g = torch.Generator().manual_seed(seed)
    ld = c + 12 if noncontiguous else c
    buf = torch.relu(torch.randn(n, H, W, ld, generator=g, dtype=torch.float32)).to(win.dtype)
    full = buf[..., :c].permute(0, 3, 1, 2)
    full[:, :, y0:y1, x0] = win
    return full


def production_inputs(seed=PRODUCTION_SEED):
    """The production-width pairwise case (C = 2560 both sides, a 16 x 32 map): post-ReLU features
    with a per-channel scale, the window of numpy seed PRODUCTION[7]."""
    n, cs, ct, h, w = PRODUCTION[:5]
    g = torch.Generator().manual_seed(seed)
    s = torch.relu(torch.randn(n, h, w, cs, generator=g)) * (torch.rand(cs, generator=g) + 0.25)
    t = torch.relu(torch.randn(n, h, w, ct, generator=g)) * (torch.rand(ct, generator=g) + 0.25)
    return s.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), window_of(h, w, PRODUCTION[7])


def loss_and_grad(fn, student, *args):
    s = student.detach().clone().requires_grad_(True)
    loss = fn(s, *args)
    loss.backward()
    return loss.detach(), s.grad.detach()
