"""AdamW on the parameter arena, the part that needs no GPU: the accept / refuse matrix of
cfg.optimizer, per-parameter chunk tables (every chunk carries its parameter's step-counter slot), the
two AdamW configs and the argument checks of the C entry points."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import util_vit as UV
from gaia_seg_amd.core import optimizer as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAMW = dict(type="AdamW", lr=6e-5)


# ---- cfg.optimizer ----
def test_adamw_cfg_accept_and_refuse_matrix():
    opt = O.check_optimizer_cfg(ADAMW)
    assert opt["betas"] == (0.9, 0.999) and opt["eps"] == 1e-8 and opt["weight_decay"] == 0.01
    opt = O.check_optimizer_cfg(dict(ADAMW, betas=[0.8, 0.99], eps=1e-6, weight_decay=0.05,
                                     paramwise_cfg=dict(norm_decay_mult=0.)))
    assert opt["betas"] == (0.8, 0.99) and opt["eps"] == 1e-6 and opt["weight_decay"] == 0.05
    assert O.check_optimizer_cfg(dict(ADAMW, weight_decay=0.0))["weight_decay"] == 0.0
    # switches that choose between torch implementations of one update, at values that change nothing
    O.check_optimizer_cfg(dict(ADAMW, amsgrad=False, maximize=False, foreach=None, capturable=False, fused=None))
    O.check_optimizer_cfg(dict(ADAMW, foreach=True, fused=False, capturable=True))
    for key in ("amsgrad", "maximize"):
        with pytest.raises(NotImplementedError, match=key):
            O.check_optimizer_cfg(dict(ADAMW, **{key: True}))
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5)):
        with pytest.raises(ValueError, match="betas"):
            O.check_optimizer_cfg(dict(ADAMW, betas=betas))
    with pytest.raises(ValueError, match="betas"):
        O.check_optimizer_cfg(dict(ADAMW, betas=0.9))
    for eps in (0.0, -1e-8):
        with pytest.raises(ValueError, match="eps"):
            O.check_optimizer_cfg(dict(ADAMW, eps=eps))
    # SGD's keys are refused by name (tests/test_paramwise.py relies on the momentum one)
    for key, val in (("momentum", 0.9), ("nesterov", False), ("dampening", 0)):
        with pytest.raises(NotImplementedError, match=key):
            O.check_optimizer_cfg(dict(ADAMW, **{key: val}))
    with pytest.raises(NotImplementedError):
        O.check_optimizer_cfg(dict(type="AdamW", lr=0.01, momentum=0.9, weight_decay=5e-4))
    for kind in ("Adam", "RMSprop", "Lamb"):
        with pytest.raises(NotImplementedError):
            O.check_optimizer_cfg(dict(type=kind, lr=0.01))
    with pytest.raises(KeyError):
        O.check_optimizer_cfg(dict(type="SGD", lr=0.01, betas=(0.9, 0.999)))
    with pytest.raises(KeyError):
        O.check_optimizer_cfg(dict(ADAMW, beta1=0.9))
    with pytest.raises(NotImplementedError, match="layer-wise"):
        O.check_optimizer_cfg(dict(ADAMW, constructor="LearningRateDecayOptimizerConstructor"))
    assert "constructor" not in O.check_optimizer_cfg(dict(ADAMW, constructor="DefaultOptimizerConstructor"))
    # SGD is what it was: nothing filled in, nothing new accepted
    sgd = dict(type="SGD", lr=0.01, momentum=0.9)
    assert O.check_optimizer_cfg(sgd) == sgd


def _seq():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 20, 3), nn.BatchNorm2d(20), nn.Conv2d(20, 40, 3), nn.BatchNorm2d(40),
                        nn.Conv2d(40, 90, 3, bias=False), nn.Conv2d(90, 8, 1))
    for p in net[2].parameters():
        p.requires_grad = False                 # a frozen layer in the middle
    return net


def test_adamw_always_has_groups_and_sgd_keeps_the_ungrouped_path():
    net = _seq()
    pg = O.build_param_groups(net, ADAMW)
    assert pg is not None and pg.groups == [(1., 1.)]
    assert set(pg.index) == {n for n, p in net.named_parameters() if p.requires_grad}
    assert O.build_param_groups(net, dict(type="SGD", lr=0.01)) is None
    assert O.build_param_groups(net, dict(type="SGD", lr=0.01, paramwise_cfg=dict())) is None
    pg = O.build_param_groups(net, dict(ADAMW, paramwise_cfg=dict(norm_decay_mult=0., bias_lr_mult=2.)))
    assert pg.groups == [(1., 1.), (2., 1.), (1., 0.)]


# ---- per-parameter tables ----
def _naive_table(fragments, chunk):
    """chunk_table restated as a loop: the reference the vectorised form is compared with, bit for bit"""
    rows = []
    for fr in fragments:
        b, e, g = fr[:3]
        while b < e:
            n = min(chunk, e - b)
            rows.append((b // 4, n // 4, g, fr[3] if len(fr) == 4 else 0))
            b += n
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def _check_per_param(model, index, chunk):
    from gaia_seg_amd.core.param_arena import arena_layout
    layout, numel = arena_layout(model)
    names = [n for n, *_ in layout]
    segs = O.segment_groups(layout, index, 64, per_param=True)
    assert [s[3] for s in segs] == list(range(len(layout)))
    # every trainable parameter, as maximal runs of neighbouring segments
    ranges = []
    for b, e, g, _ in segs:
        if g < 0:
            continue
        if ranges and ranges[-1][1] == b:
            ranges[-1][1] = e
        else:
            ranges.append([b, e])
    ranges = [tuple(r) for r in ranges]
    cache = O.ChunkTableCache(segs, chunk, numel=numel, n_slots=len(layout))
    tab, n_chunks, n_frags = cache.get(ranges)
    assert n_frags == len(index) and n_chunks == len(tab) >= n_frags
    seg_of = {s[3]: s for s in segs}
    seen, last = set(), None
    for b4, l4, g, slot in tab.tolist():
        sb, se, sg, _ = seg_of[slot]
        assert sb <= 4 * b4 and 4 * (b4 + l4) <= se and 0 < 4 * l4 <= chunk     # inside ONE parameter
        assert g == sg == index[names[slot]]                                 # (frozen ones have no index)
        if slot != last:
            assert slot not in seen                                          # contiguous per parameter
            seen.add(slot)
            last = slot
    assert seen == {i for i, n in enumerate(names) if n in index}
    covered = np.zeros(numel, dtype=np.int32)
    for b4, l4, _, _ in tab.tolist():
        covered[4 * b4:4 * (b4 + l4)] += 1
    want = np.zeros(numel, dtype=np.int32)
    for b, e, g, _ in segs:
        if g >= 0:
            want[b:e] = 1
    assert (covered == want).all()                                           # once each, frozen / gaps never
    assert np.array_equal(tab, _naive_table(O.group_fragments(ranges, segs), chunk))
    # a range over a frozen parameter is an error, so is a table that leaves the arena or the counters
    frozen = [s for s in segs if s[2] < 0]
    if frozen:
        with pytest.raises(ValueError, match="frozen"):
            cache.get([(frozen[0][0], frozen[0][1])])
    with pytest.raises(ValueError, match="leaves the arena"):
        O.ChunkTableCache(segs, chunk, numel=numel - 64, n_slots=len(layout)).get(ranges)
    with pytest.raises(ValueError, match="step counter"):
        O.ChunkTableCache(segs, chunk, numel=numel, n_slots=len(layout) - 1).get(ranges)
    return tab, segs, ranges


@pytest.mark.parametrize("chunk", [256, 4096])
def test_per_parameter_tables_on_a_small_sequential(chunk):
    net = _seq()
    pg = O.build_param_groups(net, dict(ADAMW, paramwise_cfg=dict(norm_decay_mult=0.)))
    assert not any(n.startswith("2.") for n in pg.index)
    tab, segs, ranges = _check_per_param(net, pg.index, chunk)
    # neighbours of one group are NOT merged: conv weight and conv bias (both (1, 1)) are two fragments
    frags = O.group_fragments(ranges, segs)
    assert frags[0][:3] == (segs[0][0], segs[0][1], 0) and frags[1][:3] == (segs[1][0], segs[1][1], 0)
    # ... while the SGD mode merges them, and its tables are what they have always been
    sgd_segs = O.segment_groups(arena_layout_of(net), pg.index, 64)
    assert all(len(s) == 3 for s in sgd_segs)
    sgd_frags = O.group_fragments(ranges, sgd_segs)
    assert len(sgd_frags) < len(frags) and all(len(f) == 3 for f in sgd_frags)
    sgd_tab = O.chunk_table(sgd_frags, chunk)
    assert np.array_equal(sgd_tab, _naive_table(sgd_frags, chunk)) and not sgd_tab[:, 3].any()


def arena_layout_of(model):
    from gaia_seg_amd.core.param_arena import arena_layout
    return arena_layout(model)[0]


def test_sgd_tables_are_bit_identical_to_the_known_ones():
    """The fragments of tests/test_paramwise_gpu.py, the table spelled out by a loop and two rows by hand."""
    frags = [(0, 128, 1), (128, 128 + 2 * 16384 + 192, 0), (33152, 33280, 2), (33280, 33408, 3),
             (33472, 38592, 0), (38592, 38720, 2), (38848, 38848 + 16384 + 64, 3), (55296, 59392 + 4, 1),
             (59456, 59456 + 4096, 2)]
    for chunk in (4096, 16384):
        tab = O.chunk_table(frags, chunk)
        assert tab.dtype == np.int32 and tab.tobytes() == _naive_table(frags, chunk).tobytes()
    tab = O.chunk_table(frags, 4096)
    assert tab[0].tolist() == [0, 32, 1, 0] and tab[1].tolist() == [32, 1024, 0, 0]
    assert tab[9].tolist() == [32 + 8 * 1024, 48, 0, 0] and len(tab) == 1 + 9 + 1 + 1 + 2 + 1 + 5 + 2 + 1


def test_per_parameter_tables_on_the_tiny_vit():
    from gaia_seg_amd.models import build_segmentor
    import copy
    model = build_segmentor(copy.deepcopy(UV.tiny_model_cfg()))
    pw = dict(custom_keys={"pos_embed": dict(decay_mult=0.), "cls_token": dict(decay_mult=0.)}, norm_decay_mult=0.)
    pg = O.build_param_groups(model, dict(ADAMW, paramwise_cfg=pw))
    assert pg.groups == [(1., 1.), (1., 0.)]
    for chunk in (64, 4096):
        _check_per_param(model, pg.index, chunk)


# ---- the configs ----
@pytest.mark.parametrize("name, lr, wd", [("upernet_elastic_vit_adamw.py", 6e-5, 0.01),
                                          ("upernet_convnext_t2b_adamw.py", 1e-4, 0.05)])
def test_adamw_configs_load_build_and_group(name, lr, wd):
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.optimizer import _NORMS
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "supernet", name))
    opt = O.check_optimizer_cfg(cfg.optimizer)
    assert opt["type"] == "AdamW" and opt["lr"] == lr and opt["weight_decay"] == wd
    assert tuple(opt["betas"]) == (0.9, 0.999) and "momentum" not in opt
    lrc = dict(cfg.lr_config)
    assert lrc == dict(policy="poly", power=1.0, min_lr=0.0, by_epoch=False, warmup="linear",
                       warmup_iters=1500, warmup_ratio=1e-6)
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    pg = O.build_param_groups(model, cfg.optimizer)
    assert pg.groups == [(1., 1.), (1., 0.)]
    norm_params = set()
    for prefix, m in model.named_modules():
        if isinstance(m, _NORMS):
            norm_params |= {"%s.%s" % (prefix, n) for n, _ in m.named_parameters(recurse=False)}
    assert norm_params
    n_special = 0
    for pname, p in model.named_parameters():
        special = pname in norm_params or "pos_embed" in pname or "cls_token" in pname
        n_special += special
        assert pg.index[pname] == (1 if special else 0), pname
    assert n_special > len(norm_params) or "convnext" in name
    assert pg.weight_decays(wd) == [wd, 0.0] and pg.lrs(lr) == [lr, lr]
    # the SGD twin keeps its optimizer
    twin = Config.fromfile(os.path.join(ROOT, "configs", "supernet", name.replace("_adamw", "")))
    assert twin.optimizer["type"] == "SGD"


# ---- the C entry points ----
def test_adamw_entry_points_check_their_arguments_before_any_launch(hip_lib):
    from gaia_seg_amd.hip import lib
    assert lib.ABI_VERSION >= 20 and lib.ADAMW_HYPER_DOUBLES == 8 + 2 * lib.SGD_MAX_GROUPS
    for name in ("gs_adamw_step_groups", "gs_adamw_set_group_hyper"):
        assert name in lib.PROTOTYPES and hasattr(hip_lib, name)
    OK, ODD = 1 << 20, (1 << 20) + 4

    def step(p=OK, g=OK, m=OK, v=OK, steps=OK, n_slots=8, chunks=OK, n_chunks=4, hyper=OK):
        return hip_lib.gs_adamw_step_groups(p, g, m, v, steps, n_slots, chunks, n_chunks, hyper, 1, None)

    assert hip_lib.gs_adamw_step_groups(None, None, None, None, None, 8, None, 4, None, 0, None) == -4
    for key in ("p", "g", "m", "v", "steps", "chunks", "hyper"):
        assert step(**{key: None}) == -4, key                 # GS_E_NULL
    for key in ("p", "g", "m", "v", "chunks", "hyper"):
        assert step(**{key: ODD}) == -2, key                  # GS_E_ALIGN
    assert step(steps=OK + 2) == -2
    assert step(n_chunks=0) == -1 and step(n_chunks=-3) == -1 and step(n_slots=0) == -1   # GS_E_BADARG
    g = lib.AdamwGroups()

    def set_hyper(hyper=OK, b1=0.9, b2=0.999, eps=1e-8, n=1):
        return hip_lib.gs_adamw_set_group_hyper(hyper, b1, b2, eps, 1.0, n, g, None)

    assert set_hyper(hyper=None) == -4 and set_hyper(hyper=ODD) == -2
    assert set_hyper(n=0) == -1 and set_hyper(n=lib.SGD_MAX_GROUPS + 1) == -1
    assert set_hyper(b1=1.0) == -1 and set_hyper(b2=-0.5) == -1 and set_hyper(eps=0.0) == -1
