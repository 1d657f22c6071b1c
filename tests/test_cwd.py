"""Channel-wise distillation without a GPU: the C-ABI rows of gs_cwd_*, argument validation and the
forward's split (host arithmetic), the fp64 restatement of tests/util_cwd.py against torch autograd,
the partial-state combine the kernel relies on, and the DynamicDistiller / config plumbing."""
import ctypes
import inspect
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import util_cwd as U  # noqa: E402
from test_distiller import distiller_cfg, teacher_cfg, write_teacher  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_cwd_workspace_bytes", "gs_cwd_forward", "gs_cwd_backward", "gs_cwd_debug_partials")


def _desc(n, c, h, w, layout="nhwc", T=1.0, ld_s=None, ld_t=None):
    from gaia_seg_amd.hip import lib
    d = lib.CwdDesc()
    d.N, d.C, d.H, d.W, d.T = n, c, h, w, T
    if layout == "nhwc":
        ld_s = ld_s or U.round_up(c, 4)
        ld_t = ld_t or ld_s + 4
        d.s_sn, d.s_sc, d.s_sh, d.s_sw = h * w * ld_s, 1, w * ld_s, ld_s
        d.t_sn, d.t_sc, d.t_sh, d.t_sw = h * w * ld_t, 1, w * ld_t, ld_t
    else:
        d.s_sn, d.s_sc, d.s_sh, d.s_sw = c * h * w, h * w, w, 1
        d.t_sn, d.t_sc, d.t_sh, d.t_sw = c * h * w, h * w, w, 1
    return d


def test_header_binding_and_library_export_the_symbols():
    from gaia_seg_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "gaiaseg_hip.h")).read()
    assert "typedef struct gs_cwd_desc" in header
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header and name in lib.PROTOTYPES and hasattr(cdll, name), name
    assert ctypes.sizeof(lib.CwdDesc) == 4 * 4 + 8 * 8 + 2 * 4
    assert lib.ABI_VERSION >= 16
    assert "gs_cwd_forward" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_validation_needs_no_gpu():
    from gaia_seg_amd.hip import lib
    L = lib.load()
    fake = 1 << 12      # a non-NULL address that is never dereferenced: every call returns before a launch
    fwd = lambda d, s=fake, t=fake, a=fake, b=fake, o=fake, ws=fake, nb=1 << 30: L.gs_cwd_forward(  # noqa: E731
        ctypes.byref(d) if d is not None else None, s, t, a, b, 1.0, o, ws, nb, None)
    bwd = lambda d, s=fake, t=fake, a=fake, b=fake, g=fake, ld=20: L.gs_cwd_backward(  # noqa: E731
        ctypes.byref(d) if d is not None else None, s, t, a, b, 1.0, g, ld, None)
    assert fwd(None) == -4 and bwd(None) == -4 and L.gs_cwd_workspace_bytes(None) == 0
    assert L.gs_cwd_debug_partials(None) == -4
    for field, bad in (("N", 0), ("C", -1), ("H", 0), ("W", 0), ("T", 0.0), ("T", -1.0), ("T", float("inf")),
                       ("T", float("nan")), ("N", 70000)):
        d = _desc(2, 19, 7, 9)
        setattr(d, field, bad)
        assert fwd(d) == -1 and bwd(d) == -1, (field, bad)
        assert L.gs_cwd_workspace_bytes(ctypes.byref(d)) == 0 and L.gs_cwd_debug_partials(ctypes.byref(d)) == -1
    d = _desc(2, 19, 7, 9)
    for k in ("s", "t", "a", "b", "o", "ws"):
        assert fwd(d, **{k: None}) == -4, k
    for k in ("s", "t", "a", "b", "g"):
        assert bwd(d, **{k: None}) == -4, k
    assert bwd(d, ld=18) == -1                                   # ld below C
    need = L.gs_cwd_workspace_bytes(ctypes.byref(d))
    assert need > 0 and fwd(d, nb=need // 2) == -3               # workspace too small
    assert fwd(d, ws=fake + 4) == -2                             # and not 8-byte aligned


def test_split_is_host_arithmetic_and_the_cases_cross_it():
    from gaia_seg_amd.hip import lib
    L = lib.load()
    parts = lambda *a, **k: L.gs_cwd_debug_partials(ctypes.byref(_desc(*a, **k)))  # noqa: E731
    span = U.SPAN_C19_NHWC
    assert parts(2, 19, 1, span) == 1 and parts(2, 19, 1, span + 1) == 2
    assert parts(2, 19, 1, 1) == 1
    got = {tag: parts(*c[:5]) for tag, c in U.CASES.items()}
    assert got["c19_p63"] == 1
    n, c, h, w = U.CASES["c19_p258"][:4]
    assert span < h * w <= span + 8 and got["c19_p258"] == 2     # just above one workgroup's span
    n, c, h, w = U.CASES["c19_p517"][:4]
    k = got["c19_p517"]
    assert k >= 3 and (h * w) % -(-(h * w) // k) != 0             # a ragged last range
    assert got["c150"] >= 2 and got["nchw_c19"] >= 2 and got["large"] >= 3 and got["special"] >= 3
    # the production sizes fill the machine: N * groups * ranges workgroups
    assert parts(2, 19, 64, 128) >= 32 and 2 * 5 * parts(2, 150, 128, 128) >= 512
    # the workspace holds five floats per range and (padded) channel, and a double per class map
    d = _desc(2, 19, 11, 47)
    assert L.gs_cwd_workspace_bytes(ctypes.byref(d)) >= 2 * parts(2, 19, 11, 47) * 5 * 19 * 4 + 2 * 19 * 8


def test_cpu_tensors_fail_loudly():
    from gaia_seg_amd.hip import lib
    from gaia_seg_amd.models.losses.distill_loss import channel_distill_loss
    s = torch.randn(2, 19, 4, 4, requires_grad=True)
    with pytest.raises(lib.HipLibraryError, match="no CPU fallback"):
        channel_distill_loss(s, torch.randn(2, 19, 4, 4))


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
def test_restatement_gradient_equals_autograd(T):
    g = torch.Generator().manual_seed(3)
    s = (torch.randn(2, 5, 6, 7, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    t = torch.randn(2, 5, 6, 7, generator=g, dtype=torch.float64) * 2
    loss = U.ref_channel_loss(s, t, T, 5.0)
    loss.backward()
    want = U.ref_channel_grad(s.detach(), t, T, 5.0)
    assert float((s.grad - want).abs().max()) <= 1e-14 * float(want.abs().max())
    # the definition written out: phi by exp / sum, the loss by its double sum
    n, c, h, w = s.shape
    phi = lambda x: torch.exp(x / T) / torch.exp(x / T).sum(dim=(2, 3), keepdim=True)  # noqa: E731
    ps, pt = phi(s.detach()), phi(t)
    direct = 5.0 * T * T / (n * c) * (pt * (pt.log() - ps.log())).sum()
    assert abs(float(direct) - float(loss)) <= 1e-13 * abs(float(loss))
    assert float(U.ref_channel_loss(t, t, T, 1.0)) == 0.0


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
def test_partial_state_combine_equals_the_formula(T):
    """The five-number state of csrc/cwd.hip, cut at arbitrary points and combined in index order,
    gives the column's KL and both log-sum-exps of the definition."""
    rnd = random.Random(int(T * 10))
    g = torch.Generator().manual_seed(int(T * 10))
    P = 97
    s = (torch.randn(1, 3, 1, P, generator=g, dtype=torch.float64) * 3)
    t = (torch.randn(1, 3, 1, P, generator=g, dtype=torch.float64) * 3)
    s[0, 1, 0] = torch.arange(P, dtype=torch.float64) * 0.25     # the maximum moves at every pixel
    t[0, 2, 0] = -torch.arange(P, dtype=torch.float64) * 0.25    # ... and never
    for c in range(3):
        sv, tv = s[0, c, 0].tolist(), t[0, c, 0].tolist()
        want = float(U.ref_channel_loss(s[:, c:c + 1], t[:, c:c + 1], T, 1.0)) / (T * T)
        ps = torch.softmax(s[0, c, 0] / T, 0)
        pt = torch.softmax(t[0, c, 0] / T, 0)
        for cuts in ([], [1], [40], [13, 14], sorted(rnd.sample(range(1, P), 2)),
                     sorted(rnd.sample(range(1, P), 6))):
            edges = [0] + cuts + [P]
            st = None
            for a, b in zip(edges[:-1], edges[1:]):
                seg = U.segment_state(sv[a:b], tv[a:b], T)
                st = seg if st is None else U.combine_states(st, seg, T)
            assert abs(U.state_kl(st, T) - want) <= 1e-13 * max(1.0, abs(want)), (c, cuts)
            ls, lt = U.state_lse(st, T)
            grad = torch.exp(s[0, c, 0] / T - ls) - torch.exp(t[0, c, 0] / T - lt)
            assert float((grad - (ps - pt)).abs().max()) <= 1e-14
    # associativity: (a . b) . c == a . (b . c) to rounding
    a, b, c3 = (U.segment_state(sv[i:j], tv[i:j], T) for i, j in ((0, 20), (20, 55), (55, P)))
    left = U.combine_states(U.combine_states(a, b, T), c3, T)
    right = U.combine_states(a, U.combine_states(b, c3, T), T)
    assert abs(U.state_kl(left, T) - U.state_kl(right, T)) <= 1e-13


def test_distiller_flags_and_teacher_construction(tmp_path):
    from gaia_seg_amd.models import build_segmentor
    from gaia_seg_amd.models.segmentors.dynamic_distiller import DynamicDistiller
    params = list(inspect.signature(DynamicDistiller.__init__).parameters)
    assert params[-3:] == ["has_channel_loss", "channel_loss_temperature", "channel_loss_weight"]
    assert params.index("pairwise_loss_weight") == len(params) - 4      # appended after the existing ones
    sig = inspect.signature(DynamicDistiller.__init__).parameters
    assert (sig["has_channel_loss"].default, sig["channel_loss_temperature"].default,
            sig["channel_loss_weight"].default) == (False, 1, 1)
    ck = tmp_path / "teacher.pth"
    write_teacher(ck)
    m = build_segmentor(distiller_cfg(str(ck)))
    assert m.has_channel_loss is False and m.has_distill_loss and m.has_pairwise_loss
    off = dict(has_distill_loss=False, has_pairwise_loss=False)
    assert build_segmentor(distiller_cfg(None, **off)).teacher_segmentor is None
    # the channel loss alone needs (and builds) the teacher
    with pytest.raises(AssertionError, match="Teacher ckpt is missed"):
        build_segmentor(distiller_cfg(None, has_channel_loss=True, **off))
    m = build_segmentor(distiller_cfg(str(ck), teacher=teacher_cfg(os8=False), has_channel_loss=True,
                                      channel_loss_temperature=4, channel_loss_weight=5, **off))
    t = m.teacher_segmentor
    assert t is not None and not t.training and not any(p.requires_grad for p in t.parameters())
    assert (m.has_channel_loss, m.channel_loss_temperature, m.channel_loss_weight) == (True, 4, 5)
    assert not any(k.startswith("teacher_segmentor") for k in m.state_dict())


def test_cwd_config_parses():
    from gaia_seg_amd.core.config import Config
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller_cwd.py"))
    m = cfg.model
    assert m["type"] == "DynamicDistiller" and m["teacher_segmentor"]["type"] == "DynamicEncoderDecoder"
    assert (m["has_channel_loss"], m["channel_loss_temperature"], m["channel_loss_weight"]) == (True, 1, 5)
    assert m["has_pairwise_loss"] is False and m["has_distill_loss"] is True
    assert m["decode_head"]["type"] == "DynamicPSPHead"
    base = Config.fromfile(os.path.join(ROOT, "configs", "supernet", "pspnet_ar50to101v2_distiller.py"))
    assert "has_channel_loss" not in base.model
