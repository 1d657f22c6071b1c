"""paramwise_cfg without a GPU: the grouping rule (a reconstruction of mmcv 1.3.0's
DefaultOptimizerConstructor.add_params), the fragments and the chunk table of
gs_sgd_step_groups, the per-group schedule with warm-up, the refusals and the C-ABI's argument
checks."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

from gaia_seg_amd.core import optimizer as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "configs", "supernet")
BASE_OPT = dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=0.0005)


class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(c)


class _Net(nn.Module):
    """backbone.{conv1, bn1, layer1.0, layer4.0} + decode_head.{conv (bias), bn, conv_seg (bias)}"""

    def __init__(self):
        super().__init__()
        bb = nn.Module()
        bb.conv1, bb.bn1 = nn.Conv2d(3, 8, 3, bias=False), nn.BatchNorm2d(8)
        bb.layer1, bb.layer4 = nn.Sequential(_Block(8)), nn.Sequential(_Block(8))
        self.backbone = bb
        head = nn.Module()
        head.conv, head.bn = nn.Conv2d(8, 8, 3, bias=True), nn.GroupNorm(2, 8)
        head.conv_seg = nn.Conv2d(8, 19, 1, bias=True)
        self.decode_head = head


def _groups_by_pair(pg):
    return {pair: sorted(pg.members(g)) for g, pair in enumerate(pg.groups)}


# ---- 1. the rule ----
def test_custom_keys_longest_key_wins_and_beats_the_norm_rule():
    net = _Net()
    pw = dict(custom_keys={"head": dict(lr_mult=10.), "backbone.layer4": dict(lr_mult=2., decay_mult=0.5),
                           "backbone": dict(lr_mult=0.1)}, norm_decay_mult=0.)
    pg = O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=pw))
    assert pg.groups[0] == (1., 1.)
    by = _groups_by_pair(pg)
    assert by[(1., 1.)] == []                                    # every name holds one of the keys
    assert by[(2., .5)] == ["backbone.layer4.0.bn1.bias", "backbone.layer4.0.bn1.weight",
                            "backbone.layer4.0.conv1.weight"]   # longest key first, norm rule overridden
    assert by[(.1, 1.)] == ["backbone.bn1.bias", "backbone.bn1.weight", "backbone.conv1.weight",
                            "backbone.layer1.0.bn1.bias", "backbone.layer1.0.bn1.weight",
                            "backbone.layer1.0.conv1.weight"]
    assert by[(10., 1.)] == sorted(n for n, _ in net.named_parameters() if n.startswith("decode_head"))
    assert set(pg.index) == {n for n, _ in net.named_parameters()}
    assert pg.lrs(0.01) == [0.01 * lm for lm, _ in pg.groups]
    assert pg.weight_decays(5e-4) == [5e-4 * dm for _, dm in pg.groups]


def test_key_order_is_alphabetical_then_longest_first():
    """Two keys of one length that both match: the alphabetically first wins (sorted(sorted(keys),
    key=len, reverse=True) is stable)."""
    net = _Net()
    pw = dict(custom_keys={"conv1": dict(lr_mult=3.), "bone.": dict(lr_mult=5.)})
    by = _groups_by_pair(O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=pw)))
    assert "backbone.conv1.weight" in by[(5., 1.)] and "backbone.layer1.0.conv1.weight" in by[(5., 1.)]
    assert (3., 1.) not in by


def test_bias_and_norm_multipliers_and_frozen_parameters():
    net = _Net()
    net.backbone.conv1.weight.requires_grad = False
    net.backbone.bn1.bias.requires_grad = False
    pw = dict(bias_lr_mult=2., bias_decay_mult=0., norm_decay_mult=0.25, dwconv_decay_mult=0.5,
              bypass_duplicate=True)
    pg = O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=pw))
    by = _groups_by_pair(pg)
    # bias_* only outside norm modules; norm weight AND bias get norm_decay_mult (GroupNorm too)
    assert by[(2., 0.)] == ["decode_head.conv.bias", "decode_head.conv_seg.bias"]
    assert by[(1., .25)] == ["backbone.bn1.weight", "backbone.layer1.0.bn1.bias",
                             "backbone.layer1.0.bn1.weight", "backbone.layer4.0.bn1.bias",
                             "backbone.layer4.0.bn1.weight", "decode_head.bn.bias", "decode_head.bn.weight"]
    assert by[(1., 1.)] == ["backbone.layer1.0.conv1.weight", "backbone.layer4.0.conv1.weight",
                            "decode_head.conv.weight", "decode_head.conv_seg.weight"]
    assert "backbone.conv1.weight" not in pg.index and "backbone.bn1.bias" not in pg.index   # frozen
    assert len(pg) == 3


def _norm_param_ids(model):
    from torch.nn.modules.batchnorm import _BatchNorm
    ids = set()
    for m in model.modules():
        if isinstance(m, _BatchNorm):
            ids.update(id(p) for p in m.parameters(recurse=False))
    return ids


def _build(cfg_name):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(CFG_DIR, cfg_name))
    return cfg, build_segmentor(copy.deepcopy(cfg.model))


@pytest.fixture(scope="module")
def fcn():
    return _build("fcn_ar50to101v2_paramwise.py")


def _anchors(cfg):
    return {a["name"]: a for a in cfg.train_sampler["model_samplers"][0]["anchors"]}


def _set_arch(model, meta):
    from gaia_seg_amd.core.dynamic import fold_dict
    model.manipulate_arch(fold_dict(meta)["arch"])
    return [p for p in model.active_parameters() if p.requires_grad]


def test_in_tree_paramwise_config_groups(fcn):
    cfg, model = fcn
    pg = O.build_param_groups(model, cfg.optimizer)
    assert pg.groups == [(1., 1.), (1., 0.), (10., 1.)]
    names = [n for n, _ in model.named_parameters()]
    heads = [n for n in names if "head" in n]
    assert heads and all(n.startswith(("decode_head.", "auxiliary_head.")) for n in heads)
    assert sorted(pg.members(2)) == sorted(heads)         # head norms too: custom beats norm_decay_mult
    norm_ids = _norm_param_ids(model)
    bb_norm = [n for n, p in model.named_parameters() if id(p) in norm_ids and "head" not in n]
    assert sorted(pg.members(1)) == sorted(bb_norm)
    assert len(pg.members(0)) + len(pg.members(1)) + len(pg.members(2)) == len(names) == 418
    # norm parameters per anchor against an independent module walk (MAX: 276 of 418 parameters)
    idx = {id(p): pg.index[n] for n, p in model.named_parameters()}
    only_norm = O.build_param_groups(model, dict(BASE_OPT, paramwise_cfg=dict(norm_decay_mult=0.)))
    assert only_norm.groups == [(1., 1.), (1., 0.)]
    counts = {}
    for name, meta in _anchors(cfg).items():
        active = _set_arch(model, meta)
        walk = sum(1 for p in active if id(p) in norm_ids)
        by_rule = sum(1 for n, p in model.named_parameters()
                      if only_norm.index[n] == 1 and any(p is q for q in active))
        assert walk == by_rule, name
        counts[name] = (walk, len(active))
        assert all(id(p) in idx for p in active)
    assert counts["MAX"] == (276, 418)
    assert counts["MIN"][0] < counts["R50"][0] < counts["R77"][0] < counts["R101"][0] < 276


# ---- 2. fragments and the chunk table ----
def _ranges(layout, params):
    seg = {id(p): (o, -(-max(n, 1) // 64) * 64) for _n, p, _ph, o, n in layout}
    merged = []
    for o, n in sorted(seg[id(p)] for p in params):
        if merged and merged[-1][1] == o:
            merged[-1][1] = o + n
        else:
            merged.append([o, o + n])
    return [tuple(r) for r in merged]


def _check_table(tab, ranges, segs, ch):
    """Chunks are disjoint, cover exactly ``ranges``, lie in one group each, none exceeds ``ch``."""
    assert tab.dtype == np.int32 and tab.shape[1] == 4 and (tab[:, 3] == 0).all()
    b, n, g = tab[:, 0].astype(np.int64) * 4, tab[:, 1].astype(np.int64) * 4, tab[:, 2]
    assert (n > 0).all() and (n <= ch).all()
    order = np.argsort(b)
    b, n, g = b[order], n[order], g[order]
    assert (b[1:] >= (b + n)[:-1]).all()                       # disjoint
    cover = []                                                  # union of the chunks
    for lo, hi in zip(b.tolist(), (b + n).tolist()):
        if cover and cover[-1][1] == lo:
            cover[-1][1] = hi
        else:
            cover.append([lo, hi])
    assert [tuple(c) for c in cover] == list(ranges)
    starts = np.array([s[0] for s in segs])
    ends = np.array([s[1] for s in segs])
    sgrp = np.array([s[2] for s in segs])
    first = np.searchsorted(starts, b, side="right") - 1       # segment holding the chunk's first float
    last = np.searchsorted(starts, b + n - 1, side="right") - 1
    assert (sgrp[first] == g).all() and (sgrp[last] == g).all()
    for i in np.nonzero(first != last)[0]:                      # a chunk over several segments: one group
        assert (sgrp[first[i]:last[i] + 1] == g[i]).all()
    assert (b + n <= ends[last]).all()


# merged ranges per step without groups / fragments once norm parameters are their own group
FRAGMENTS = {
    "fcn_ar50to101v2.py": {"MAX": (1, 276), "R101": (5, 216), "R50": (5, 114), "MIN": (5, 84)},
    "pspnet_ar50to101v2.py": {"MAX": (1, 280), "R101": (5, 220), "R50": (5, 118), "MIN": (5, 88)},
    "upernet_ar50to101v2.py": {"MAX": (1, 294), "R101": (5, 234), "R50": (5, 132), "MIN": (5, 102)},
}


@pytest.mark.parametrize("cfg_name", sorted(FRAGMENTS))
def test_fragment_counts_of_the_in_tree_supernets(cfg_name):
    from gaia_seg_amd.core.param_arena import arena_layout
    cfg, model = _build(cfg_name)
    layout, total = arena_layout(model)
    pg = O.build_param_groups(model, dict(BASE_OPT, paramwise_cfg=dict(norm_decay_mult=0.)))
    segs = O.segment_groups(layout, pg.index)
    assert segs[-1][1] == total
    for name, meta in _anchors(cfg).items():
        ranges = _ranges(layout, _set_arch(model, meta))
        frags = O.group_fragments(ranges, segs)
        if name in FRAGMENTS[cfg_name]:
            assert (len(ranges), len(frags)) == FRAGMENTS[cfg_name][name], name
        assert min(e - b for b, e, _ in frags) >= 64
        for ch in (4096, 16384, 65536):
            _check_table(O.chunk_table(frags, ch), ranges, segs, ch)


def test_chunk_tables_of_anchors_and_sampled_subnets(fcn):
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.param_arena import arena_layout
    cfg, model = fcn
    layout, _ = arena_layout(model)
    pg = O.build_param_groups(model, cfg.optimizer)
    segs = O.segment_groups(layout, pg.index)
    base_frags = {}
    only_norm = O.segment_groups(layout, O.build_param_groups(
        model, dict(BASE_OPT, paramwise_cfg=dict(norm_decay_mult=0.))).index)
    sampler = build_model_sampler(copy.deepcopy(cfg.train_sampler))
    sampler.seed(1234)
    metas = list(_anchors(cfg).values()) + [sampler.sample() for _ in range(50)]
    assert len({str(m) for m in metas}) > 10      # (the sampler also returns its anchors)
    for meta in metas:
        ranges = _ranges(layout, _set_arch(model, meta))
        frags = O.group_fragments(ranges, segs)
        assert {g for _, _, g in frags} == {0, 1, 2}
        assert all(b % 64 == 0 and e % 64 == 0 for b, e, _ in frags)
        # the 'head' key adds no fragment: the heads sit at the end of the arena
        assert len(frags) <= len(O.group_fragments(ranges, only_norm))
        tab = O.chunk_table(frags)
        _check_table(tab, ranges, segs, O.CHUNK_FLOATS)
        assert len(tab) == sum(-(-(e - b) // O.CHUNK_FLOATS) for b, e, _ in frags)
        base_frags[meta.get("name", "random")] = len(frags)
    assert base_frags["MAX"] <= 276


def test_fragment_and_chunk_edge_cases():
    segs = [(0, 64, 0), (64, 192, 1), (192, 256, 1), (256, 320, -1), (320, 448, 0), (448, 512, 2)]
    assert O.group_fragments([(0, 256)], segs) == [(0, 64, 0), (64, 256, 1)]
    assert O.group_fragments([(0, 64), (320, 512)], segs) == [(0, 64, 0), (320, 448, 0), (448, 512, 2)]
    assert O.group_fragments([(64, 192), (192, 256)], segs) == [(64, 256, 1)]
    with pytest.raises(ValueError):
        O.group_fragments([(192, 320)], segs)                 # a frozen segment inside a stepped range
    with pytest.raises(ValueError):
        O.group_fragments([(32, 64)], segs)
    with pytest.raises(ValueError):
        O.group_fragments([(0, 100)], segs)
    tab = O.chunk_table([(0, 64, 0), (64, 256, 1)], 128)
    assert tab.tolist() == [[0, 16, 0, 0], [16, 32, 1, 0], [48, 16, 1, 0]]   # 192 = 128 + a 64 tail
    assert O.chunk_table([], 128).shape == (0, 4)
    with pytest.raises(ValueError):
        O.chunk_table([(0, 64, 0)], 6)
    with pytest.raises(ValueError):
        O.chunk_table([(2, 66, 0)], 64)


# ---- 3. the schedule ----
class _R:
    """What an lr updater hook touches of a runner."""

    def __init__(self, base_lr, max_iters, mults=None):
        self.base_lr = self.lr = base_lr
        self.max_iters, self.iter = max_iters, 0
        if mults is not None:
            self.group_base_lr = [base_lr * m for m in mults]
            self.group_lr = list(self.group_base_lr)


def test_per_group_poly_schedule_starts_from_each_groups_own_lr():
    from gaia_seg_amd.core.runner import PolyLrUpdaterHook
    T, base, min_lr, power = 1000, 0.01, 1e-4, 0.9
    r = _R(base, T, mults=[1., 1., 10.])
    h = PolyLrUpdaterHook(power=power, min_lr=min_lr, by_epoch=False)
    h.before_run(r)
    for t in (0, T // 2, T - 1):
        r.iter = t
        h.before_train_iter(r)
        c = (1 - t / T) ** power
        want = [(0.01 - 1e-4) * c + 1e-4, (0.01 - 1e-4) * c + 1e-4, (0.1 - 1e-4) * c + 1e-4]
        assert r.group_lr == pytest.approx(want, rel=1e-12)
        assert r.lr == r.group_lr[0]
        if t:   # with min_lr the head's lr is NOT 10 x the base group's
            assert abs(r.group_lr[2] - 10 * r.group_lr[0]) > 1e-5
    # a runner without groups: exactly the one-lr schedule, no group attribute appears
    r1 = _R(base, T)
    h.before_run(r1)
    r1.iter = 500
    h.before_train_iter(r1)
    assert r1.lr == (base - min_lr) * (1 - 500 / T) ** power + min_lr and not hasattr(r1, "group_lr")


@pytest.mark.parametrize("form", ["constant", "linear", "exp"])
def test_warmup_forms(form):
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, PolyLrUpdaterHook
    T, W, ratio, base, min_lr, power = 1000, 100, 1e-3, 0.01, 1e-4, 0.9
    h = PolyLrUpdaterHook(power=power, min_lr=min_lr, warmup=form, warmup_iters=W, warmup_ratio=ratio)
    r = _R(base, T, mults=[1., 10.])
    h.before_run(r)

    def regular(b, t):
        return (b - min_lr) * (1 - t / T) ** power + min_lr

    def factor(t):
        if form == "constant":
            return ratio
        if form == "linear":
            return 1 - (1 - t / W) * (1 - ratio)
        return ratio ** (1 - t / W)

    for t in (0, W // 2, W - 1):
        r.iter = t
        h.before_train_iter(r)
        assert r.group_lr == pytest.approx([regular(0.01, t) * factor(t), regular(0.1, t) * factor(t)],
                                           rel=1e-12)
    assert factor(0) == pytest.approx(ratio)
    for t in (W, W + 1):        # from warmup_iters on: the regular lr, nothing else
        r.iter = t
        h.before_train_iter(r)
        assert r.group_lr == [regular(0.01, t), regular(0.1, t)] and r.lr == regular(0.01, t)
    if form != "constant":      # no jump after the last warm-up step beyond the formula's own
        r.iter = W - 1
        h.before_train_iter(r)
        assert abs(r.lr - regular(0.01, W)) / regular(0.01, W) < (0.07 if form == "exp" else 0.011)
    # warm-up without groups only changes runner.lr; the fixed policy warms up too
    r1 = _R(base, T)
    f = FixedLrUpdaterHook(warmup=form, warmup_iters=W, warmup_ratio=ratio)
    f.before_run(r1)
    for t in (0, W // 2, W):
        r1.iter = t
        f.before_train_iter(r1)
        assert r1.lr == pytest.approx(base * (factor(t) if t < W else 1.), rel=1e-12)


def test_hooks_built_as_bench_and_tests_build_them_are_unchanged():
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, PolyLrUpdaterHook
    r = _R(0.05, 100)
    h = PolyLrUpdaterHook(power=0.9, min_lr=1e-4)
    h.before_run(r)
    for t in (0, 3, 99):
        r.iter = t
        h.before_train_iter(r)
        assert r.lr == (0.05 - 1e-4) * (1 - t / 100) ** 0.9 + 1e-4 == h.get_lr(r)
    f = FixedLrUpdaterHook()
    r.iter = 7
    f.before_train_iter(r)
    assert r.lr == 0.05


# ---- 4. refusals ----
def test_refusals():
    from gaia_seg_amd.core.runner import FixedLrUpdaterHook, PolyLrUpdaterHook
    net = nn.Sequential(*[nn.Linear(4, 4) for _ in range(10)])
    names = [n for n, _ in net.named_parameters()]
    many = {n: dict(lr_mult=2. + i) for i, n in enumerate(names)}
    assert len(many) >= O.MAX_GROUPS
    with pytest.raises(ValueError, match="GS_SGD_MAX_GROUPS"):
        O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(custom_keys=many)))
    few = dict(list(many.items())[:O.MAX_GROUPS - 1])          # 15 custom groups + (1, 1): allowed
    assert len(O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(custom_keys=few)))) == O.MAX_GROUPS
    with pytest.raises(NotImplementedError, match="nesterov"):
        O.build_param_groups(net, dict(BASE_OPT, nesterov=True))
    with pytest.raises(NotImplementedError, match="dampening"):
        O.check_optimizer_cfg(dict(BASE_OPT, dampening=0.1))
    assert O.check_optimizer_cfg(dict(BASE_OPT, nesterov=False, dampening=0))["lr"] == 0.01
    with pytest.raises(KeyError):
        O.check_optimizer_cfg(dict(BASE_OPT, betas=(0.9, 0.999)))
    with pytest.raises(NotImplementedError):
        O.check_optimizer_cfg(dict(BASE_OPT, type="AdamW"))
    with pytest.raises(NotImplementedError, match="dcn_offset_lr_mult"):
        O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(dcn_offset_lr_mult=0.1)))
    with pytest.raises(KeyError):
        O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(norm_lr_mult=0.1)))
    with pytest.raises(KeyError):
        O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(custom_keys={"head": dict(lr=1.)})))
    with pytest.raises(NotImplementedError, match="warmup_by_epoch"):
        PolyLrUpdaterHook(power=0.9, warmup="linear", warmup_iters=5, warmup_by_epoch=True)
    with pytest.raises(KeyError):
        PolyLrUpdaterHook(power=0.9, min_lr=1e-4, gamma=0.1)
    with pytest.raises(KeyError):
        FixedLrUpdaterHook(step=[10])
    with pytest.raises(ValueError):
        PolyLrUpdaterHook(warmup="cosine", warmup_iters=5)
    with pytest.raises(ValueError):
        PolyLrUpdaterHook(warmup="linear", warmup_iters=0)
    with pytest.raises(ValueError):
        PolyLrUpdaterHook(warmup="linear", warmup_iters=5, warmup_ratio=0.)


def test_no_paramwise_cfg_yields_no_grouping(fcn):
    from gaia_seg_amd.core.config import Config
    net = _Net()
    assert O.build_param_groups(net, BASE_OPT) is None
    assert O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict())) is None
    assert O.build_param_groups(net, dict(BASE_OPT, paramwise_cfg=dict(norm_decay_mult=1.,
                                                                       bias_lr_mult=1.))) is None
    plain = Config.fromfile(os.path.join(CFG_DIR, "fcn_ar50to101v2.py"))
    assert O.build_param_groups(fcn[1], plain.optimizer) is None
    cfg = fcn[0]
    assert cfg.optimizer.paramwise_cfg.custom_keys == {"head": {"lr_mult": 10.}}
    assert cfg.lr_config.warmup == "linear" and cfg.lr_config.warmup_iters == 500
    assert {k: v for k, v in cfg.optimizer.items() if k != "paramwise_cfg"} == dict(plain.optimizer)


# ---- 5. the C-ABI ----
def test_group_sgd_symbols_and_argument_checks_need_no_gpu():
    from gaia_seg_amd.hip import lib
    L = lib.load()
    assert lib.ABI_VERSION >= 11 and lib.SGD_MAX_GROUPS == O.MAX_GROUPS == 16
    for name in ("gs_sgd_set_group_hyper", "gs_sgd_step_groups"):
        assert name in lib.PROTOTYPES and hasattr(ctypes.CDLL(lib.LIB_PATH), name)
    assert ctypes.sizeof(lib.SgdChunk) == 16 and ctypes.sizeof(lib.SgdGroups) == 2 * 16 * 4
    header = open(os.path.join(ROOT, "include", "gaiaseg_hip.h")).read()
    assert "#define GS_SGD_MAX_GROUPS 16" in header
    g = lib.SgdGroups()
    a = 0x1000                     # any 16-byte aligned non-null address: refused calls launch nothing
    assert L.gs_sgd_set_group_hyper(None, 0.9, 1.0, 2, g, None) == -4
    assert L.gs_sgd_set_group_hyper(a, 0.9, 1.0, 0, g, None) == -1
    assert L.gs_sgd_set_group_hyper(a, 0.9, 1.0, lib.SGD_MAX_GROUPS + 1, g, None) == -1
    assert L.gs_sgd_set_group_hyper(a + 4, 0.9, 1.0, 2, g, None) == -2
    for bad in range(3):
        ptrs = [a, a, a]
        ptrs[bad] = None
        assert L.gs_sgd_step_groups(*ptrs, a, 4, a, 1, None) == -4
    assert L.gs_sgd_step_groups(a, a, a, None, 4, a, 1, None) == -4
    assert L.gs_sgd_step_groups(a, a, a, a, 4, None, 1, None) == -4
    assert L.gs_sgd_step_groups(a, a, a, a, 0, a, 1, None) == -1
    assert L.gs_sgd_step_groups(a, a, a, a, -3, a, 1, None) == -1
    assert L.gs_sgd_step_groups(a, a, a, a + 8, 4, a, 1, None) == -2      # misaligned table
    assert L.gs_sgd_step_groups(a, a, a, a, 4, a + 4, 1, None) == -2
    assert L.gs_sgd_step_groups(a + 4, a, a, a, 4, a, 1, None) == -2


# ---- 6. the table cache ----
def test_table_cache_evicts_one_by_one_and_never_what_a_holder_or_the_current_subnet_uses():
    """More than 512 range sets go through the cache (a run draws random subnets for 80000
    iterations): entries leave one at a time, oldest first; the tables of the subnet being prepared
    are never among them; a table somebody holds (a captured step graph) stays the object it was,
    with its contents; an evicted set of ranges is rebuilt equal."""
    segs = [(64 * i, 64 * (i + 1), (i % 3 == 1) + 2 * (i % 7 == 3)) for i in range(64)]
    uploads = []

    def upload(tab):
        uploads.append(tab.copy())
        return uploads[-1]

    cache = O.ChunkTableCache(segs, chunk_floats=64, upload=upload, max_entries=512)
    sets = [((64 * i, 64 * j),) for i in range(64) for j in range(i + 1, 65)]       # 2080 range sets
    assert len(sets) > 4 * 512
    anchors = sets[:3]                                      # "the anchors' graphs" hold these
    held = [cache.get(r) for r in anchors]
    snapshot = [h[0].copy() for h in held]
    for n, r in enumerate(sets[3:], 3):
        # a subnet prepares three tables in a row (whole step, early, late), then steps with them
        trio = [r, (r[0], (4032, 4096)) if r[0][1] < 4032 else r, ((0, 64), r[0]) if r[0][0] > 64 else r]
        got = [cache.get(t) for t in trio]
        assert all(t in cache for t in trio), n                                   # none evicted by a sibling
        assert [cache.get(t, build=False)[0] is g[0] for t, g in zip(trio, got)] == [True] * 3
        assert len(cache) <= 512
    assert len(cache) == 512 and len(uploads) > 2080
    assert not any(a in cache for a in anchors)                                   # long evicted ...
    for h, snap, r in zip(held, snapshot, anchors):
        assert np.array_equal(h[0], snap)                                         # ... and untouched
        again = cache.get(r)
        assert again[0] is not h[0] and np.array_equal(again[0], snap) and again[1:] == h[1:]
    with pytest.raises(KeyError):
        cache.get(sets[5], build=False)
    # least recently USED, not least recently inserted: a fetched entry moves to the back
    small = O.ChunkTableCache(segs, chunk_floats=64, max_entries=8)
    for r in sets[:8]:
        small.get(r)
    small.get(sets[0])
    small.get(sets[8])
    assert sets[0] in small and sets[1] not in small and len(small) == 8
    with pytest.raises(ValueError):
        O.ChunkTableCache(segs, max_entries=2)
    with pytest.raises(ValueError, match="leaves the arena"):
        O.ChunkTableCache(segs, chunk_floats=64, numel=1024).get(((0, 2048),))
