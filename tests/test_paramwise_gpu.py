"""paramwise_cfg on the GPU: gs_sgd_step_groups against torch.optim.SGD with the same param groups,
bitwise against gs_sgd_step for a (1, 1) group, untouched elements outside the table, and the runner
(per-group schedule with warm-up, step graphs, launch counts, the sandwich iteration, the CLI)."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from util_models import arch_meta, fcn_head, make_batch, model_cfg, psp_head

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

BASE_LR, BASE_WD, MOM = 0.01, 5e-4, 0.9
MULTS = [(1., 1.), (10., 1.), (1., 0.), (0., 1.)]
# (begin, end, group) in floats: 128-float fragments, fragments that end off a chunk boundary
# (4096 / 16384), gaps that are in no chunk, the last fragment ending 64 floats before the arena's end
FRAGS = [(0, 128, 1), (128, 128 + 2 * 16384 + 192, 0), (33152, 33280, 2), (33280, 33408, 3),
         (33472, 38592, 0), (38592, 38720, 2), (38848, 38848 + 16384 + 64, 3), (55296, 59392 + 4, 1),
         (59456, 59456 + 4096, 2)]
ZERO_GRAD_FRAG = 5          # the (1, 0) fragment that is fed zero gradients
NUMEL = 59456 + 4096 + 64


def _stream():
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    return current_stream_ptr()


def _set_hyper(L, hyper, lrs, wds, momentum=MOM, gscale=1.0):
    from gaia_seg_amd.hip import lib
    g = lib.SgdGroups()
    for i, (lr, wd) in enumerate(zip(lrs, wds)):
        g.lr_wd[2 * i], g.lr_wd[2 * i + 1] = lr, wd
    lib.check(L.gs_sgd_set_group_hyper(hyper.data_ptr(), momentum, gscale, len(lrs), g, _stream()),
              "gs_sgd_set_group_hyper")


def _table(frags, ch):
    from gaia_seg_amd.core.optimizer import chunk_table
    tab = chunk_table(frags, ch)
    assert int((tab[:, 0].astype(np.int64) + tab[:, 1]).max()) * 4 <= NUMEL       # bounds, before any launch
    return torch.from_numpy(tab).to(DEV), len(tab)


def _mask(frags, group=None):
    m = torch.zeros(NUMEL, dtype=torch.bool)
    for b, e, g in frags:
        if group is None or g == group:
            m[b:e] = True
    return m


def _bits(t):
    return t.detach().cpu().view(torch.int32)


@pytest.mark.parametrize("ch", [4096, 16384])
def test_group_sgd_matches_torch_param_groups(hip_lib, ch):
    """Three steps, momentum 0.9, zero_grad alternating, four groups (1,1) (10,1) (1,0) (0,1):
    rel_err < 1e-6 per group (test_sgd_step_matches_torch's bound); lr = 0 leaves parameters bitwise
    alone while momentum moves; no decay + zero gradient leaves a fragment bitwise alone."""
    from gaia_seg_amd.hip import lib
    torch.manual_seed(0)
    lrs = [BASE_LR * lm for lm, _ in MULTS]
    wds = [BASE_WD * dm for _, dm in MULTS]
    table, n_chunks = _table(FRAGS, ch)
    assert n_chunks > len(FRAGS)
    p0 = torch.randn(NUMEL)
    masks = [_mask(FRAGS, g) for g in range(4)]
    inside = _mask(FRAGS)
    zf = torch.zeros(NUMEL, dtype=torch.bool)
    zf[FRAGS[ZERO_GRAD_FRAG][0]:FRAGS[ZERO_GRAD_FRAG][1]] = True
    ref = [p0[m].clone().requires_grad_(True) for m in masks]
    opt = torch.optim.SGD([dict(params=[ref[g]], lr=lrs[g], weight_decay=wds[g]) for g in range(4)],
                          lr=BASE_LR, momentum=MOM, weight_decay=BASE_WD)
    p, mom = p0.to(DEV), torch.zeros(NUMEL, device=DEV)
    hyper = torch.zeros(4 + 2 * lib.SGD_MAX_GROUPS, device=DEV)
    _set_hyper(hip_lib, hyper, lrs, wds)
    for step in range(3):
        g = torch.randn(NUMEL)
        g[zf] = 0.
        for k in range(4):
            ref[k].grad = g[masks[k]].clone()
        opt.step()
        gg = g.to(DEV)
        zero = step % 2
        lib.check(hip_lib.gs_sgd_step_groups(p.data_ptr(), gg.data_ptr(), mom.data_ptr(), table.data_ptr(),
                                             n_chunks, hyper.data_ptr(), zero, _stream()), "groups")
        torch.cuda.synchronize()
        if zero:   # cleared inside the table, untouched outside
            assert float(gg.cpu()[inside].abs().max()) == 0.0
            assert torch.equal(_bits(gg)[~inside], _bits(g)[~inside])
        else:
            assert torch.equal(_bits(gg), _bits(g))
    pc, mc = p.cpu(), mom.cpu()
    for k in range(4):
        err = rel_err(pc[masks[k]], ref[k])
        merr = rel_err(mc[masks[k]], opt.state[ref[k]]["momentum_buffer"])
        print("group %d %s: param rel_err %.3e, momentum rel_err %.3e" % (k, MULTS[k], err, merr))
        assert err < 1e-6 and merr < 1e-6, (k, err, merr)
    assert torch.equal(_bits(pc)[masks[3]], _bits(p0)[masks[3]])          # lr_mult 0: bitwise unchanged
    assert float(mc[masks[3]].abs().min()) > 0                            # ... while its momentum moved
    assert torch.equal(_bits(pc)[zf], _bits(p0)[zf])                      # (1, 0) with zero gradients
    assert float(mc[zf].abs().max()) == 0.0
    assert not torch.equal(pc[masks[2] & ~zf], p0[masks[2] & ~zf])
    assert float(hyper[2]) == 4.0 and hyper[4:12].cpu().tolist() == pytest.approx(
        [v for pair in zip(lrs, wds) for v in pair], rel=1e-7)


def test_single_group_is_bitwise_gs_sgd_step(hip_lib):
    """One group (1, 1): parameters, momentum and cleared gradients equal gs_sgd_step over the same
    ranges bit for bit (both kernels evaluate one __device__ function)."""
    from gaia_seg_amd.hip import lib
    torch.manual_seed(1)
    frags = [(b, e, 0) for b, e, _ in FRAGS]
    table, n_chunks = _table(frags, 4096)
    hyper = torch.zeros(4 + 2 * lib.SGD_MAX_GROUPS, device=DEV)
    lr, wd, gscale = 0.0123, 5e-4, 1.0 / 512
    _set_hyper(hip_lib, hyper, [lr], [wd], MOM, gscale)
    pa = torch.randn(NUMEL, device=DEV)
    pb = pa.clone()
    ma, mb = torch.zeros(NUMEL, device=DEV), torch.zeros(NUMEL, device=DEV)
    for step in range(3):
        ga = torch.randn(NUMEL, device=DEV) * 512
        gb = ga.clone()
        zero = (step + 1) % 2
        lib.check(hip_lib.gs_sgd_step_groups(pa.data_ptr(), ga.data_ptr(), ma.data_ptr(), table.data_ptr(),
                                             n_chunks, hyper.data_ptr(), zero, _stream()), "groups")
        for b, e, _ in frags:
            lib.check(hip_lib.gs_sgd_step(pb.data_ptr() + 4 * b, gb.data_ptr() + 4 * b, mb.data_ptr() + 4 * b,
                                          e - b, lr, MOM, wd, gscale, zero, _stream()), "sgd")
        torch.cuda.synchronize()
        assert torch.equal(_bits(pa), _bits(pb)), step
        assert torch.equal(_bits(ma), _bits(mb)), step
        assert torch.equal(_bits(ga), _bits(gb)), step
    assert float(ma.abs().max()) > 0


def test_elements_outside_the_table_keep_their_bits(hip_lib):
    """Canary: padding / skipped / frozen elements (everything no chunk covers) are never written in
    param, momentum or grad -- NaN patterns included -- and an entry naming a group the hyper table
    does not have is skipped."""
    from gaia_seg_amd.hip import lib
    torch.manual_seed(2)
    inside = _mask(FRAGS)
    canary = torch.randint(-2 ** 31, 2 ** 31 - 1, (NUMEL,), dtype=torch.int64).to(torch.int32)
    bufs = []
    for _ in range(3):
        t = torch.randn(NUMEL)
        t.view(torch.int32)[~inside] = canary[~inside]
        bufs.append(t)
    table, n_chunks = _table(FRAGS, 4096)
    hyper = torch.zeros(4 + 2 * lib.SGD_MAX_GROUPS, device=DEV)
    _set_hyper(hip_lib, hyper, [0.01, 0.1, 0.01, 0.02], [5e-4] * 4)
    p, g, m = (t.to(DEV) for t in bufs)
    for zero in (0, 1):
        lib.check(hip_lib.gs_sgd_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), table.data_ptr(),
                                             n_chunks, hyper.data_ptr(), zero, _stream()), "groups")
    torch.cuda.synchronize()
    for name, t, t0 in (("param", p, bufs[0]), ("grad", g, bufs[1]), ("momentum", m, bufs[2])):
        assert torch.equal(_bits(t)[~inside], _bits(t0)[~inside]), name
        assert not torch.equal(_bits(t)[inside], _bits(t0)[inside]), name
    # only two groups in the hyper table: the chunks of groups 2 and 3 are skipped, not followed
    p2, g2, m2 = (t.to(DEV) for t in bufs)
    _set_hyper(hip_lib, hyper, [0.01, 0.1], [5e-4] * 2)
    lib.check(hip_lib.gs_sgd_step_groups(p2.data_ptr(), g2.data_ptr(), m2.data_ptr(), table.data_ptr(),
                                         n_chunks, hyper.data_ptr(), 1, _stream()), "groups")
    torch.cuda.synchronize()
    low = _mask(FRAGS, 0) | _mask(FRAGS, 1)
    for t, t0 in ((p2, bufs[0]), (g2, bufs[1]), (m2, bufs[2])):
        assert torch.equal(_bits(t)[~low], _bits(t0)[~low])
        assert not torch.equal(_bits(t)[low], _bits(t0)[low])


# ---- the runner ----
OPTIMIZER = dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=0.0005,
                 paramwise_cfg=dict(custom_keys={"head": dict(lr_mult=10.)}, norm_decay_mult=0.))
LR_CONFIG = dict(power=0.9, min_lr=1e-4, by_epoch=False, warmup="linear", warmup_iters=2, warmup_ratio=1e-3)


def _anchor(name):
    a = arch_meta(name)["backbone"]
    return {"name": name, "arch.backbone.stem.width": a["stem"]["width"],
            "arch.backbone.body.width": a["body"]["width"], "arch.backbone.body.depth": a["body"]["depth"]}


def _batch(seed=0):
    img, gt = make_batch(2, 64, 96, seed=seed)
    metas = [dict(ori_shape=(64, 96, 3), img_shape=(64, 96, 3), flip=False) for _ in range(2)]
    return dict(img=img.cuda(), img_metas=metas, gt_semantic_seg=gt.cuda())


def _model(head, seed=0):
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(model_cfg(head, aux=True))).cuda().train()
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model


def _runner(model, optimizer=OPTIMIZER, lr_config=LR_CONFIG, max_iters=8, hooks=True):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, PolyLrUpdaterHook
    arena = ParamArena(model)
    pg = build_param_groups(model, optimizer)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments),
                             base_lr=optimizer["lr"], momentum=optimizer["momentum"],
                             weight_decay=optimizer["weight_decay"], max_iters=max_iters, param_groups=pg)
    runner.register_hook(PolyLrUpdaterHook(**lr_config))
    if hooks:
        runner.register_hook(ArenaOptimizerHook())
    return runner, arena, pg


class _TorchTwin:
    """torch.optim.SGD on CPU copies of the arena segments, one param group per parameter group,
    stepped with the gradients and per-group lr the arena's sgd_step was given."""

    def __init__(self, model, arena, pg, momentum=0.9):
        self.arena, self.pg = arena, pg
        flat = arena.flat_param.detach().cpu()
        self.params, self.seg = {}, {}
        for name, p in model.named_parameters():
            o, n = arena.segments[id(p)]
            self.seg[name] = (o, n)
            self.params[name] = flat[o:o + n].clone().requires_grad_(True)
        groups = [dict(params=[self.params[n] for n in pg.members(g)], lr=0.0, weight_decay=0.0)
                  for g in range(len(pg))]
        self.opt = torch.optim.SGD([g for g in groups if g["params"]], lr=0.0, momentum=momentum)
        self.group_of = {id(self.params[n]): g for n, g in pg.index.items()}
        self.calls = []
        orig = arena.sgd_step

        def recorded(ranges, lr, momentum=0.9, weight_decay=5e-4, grad_scale=1.0, zero_grad=False, hyper=None):
            self.calls.append((list(ranges), list(lr), list(weight_decay), grad_scale,
                               arena.flat_grad.detach().cpu().clone()))
            return orig(ranges, lr, momentum, weight_decay, grad_scale, zero_grad, hyper=hyper)
        arena.sgd_step = recorded

    def replay(self):
        for ranges, lrs, wds, gscale, grad in self.calls:
            for g in self.opt.param_groups:
                k = self.group_of[id(g["params"][0])]
                g["lr"], g["weight_decay"] = lrs[k], wds[k]
            for name, t in self.params.items():
                o, n = self.seg[name]
                covered = any(a <= o and o + n <= b for a, b in ranges) and name in self.pg.index
                t.grad = grad[o:o + n].clone() * gscale if covered else None
            self.opt.step()
        self.calls = []

    def worst(self):
        flat = self.arena.flat_param.detach().cpu()
        errs = {n: rel_err(flat[o:o + k], self.params[n]) for n, (o, k) in self.seg.items()}
        return max(errs.items(), key=lambda kv: kv[1])


def test_runner_steps_equal_torch_grouped_sgd(hip_lib):
    """Four steps over two subnets with the paramwise optimizer and a two-iteration linear warm-up:
    every parameter equals torch.optim.SGD with mmcv-style groups fed the same gradients and the
    hook's per-group lr (rel_err < 1e-6).  Without the feature the multipliers are ignored and this
    fails."""
    model = _model(fcn_head())
    runner, arena, pg = _runner(model)
    assert pg.groups == [(1., 1.), (1., 0.), (10., 1.)] and arena.groups == 3
    twin = _TorchTwin(model, arena, pg)
    runner.call_hook("before_run")
    seen_lr = []
    for it, name in enumerate(["sub", "min", "sub", "min"]):
        runner.set_arch(_anchor(name))
        runner.train_iter(_batch(it))
        torch.cuda.synchronize()
        seen_lr.append(list(runner.group_lr))
        assert twin.calls and all(c[1] == runner.group_lr for c in twin.calls)
        assert all(c[2] == [5e-4, 0.0, 5e-4] for c in twin.calls)
        twin.replay()
        name_w, err = twin.worst()
        print("iter %d (%s): worst parameter %s rel_err %.3e, group lr %s" % (it, name, name_w, err, runner.group_lr))
        assert err < 1e-6, (it, name_w, err)
    # the hook's schedule: warm-up over iterations 0 and 1, each group from its own initial lr
    for t, lrs in enumerate(seen_lr):
        c = (1 - t / 8) ** 0.9
        f = 1 - (1 - t / 2) * (1 - 1e-3) if t < 2 else 1.0
        want = [((b - 1e-4) * c + 1e-4) * f for b in (0.01, 0.01, 0.1)]
        assert lrs == pytest.approx(want, rel=1e-12)
    # the head moved further than one learning rate would take it, BN parameters did not decay
    assert float(arena.flat_mom.abs().max()) > 0 and arena.grads_clean


def test_grouped_step_graph_replay_is_bitwise_the_eager_run(hip_lib):
    def run(graphs):
        model = _model(fcn_head())
        runner, arena, _ = _runner(model)
        runner.graphs_enabled = graphs
        runner.call_hook("before_run")
        for it, name in enumerate(["sub", "min", "sub", "min", "sub", "sub", "min"]):
            runner.set_arch(_anchor(name))
            runner.train_iter(_batch(it))
        torch.cuda.synchronize()
        return arena.flat_param.clone(), arena.flat_mom.clone(), dict(runner.graph_stats)

    p_e, m_e, st_e = run(False)
    p_g, m_g, st_g = run(True)
    assert st_e["replayed"] == 0 and st_e["captured"] == 0
    assert st_g["replayed"] > 0 and st_g["captured"] == 2, st_g
    assert torch.equal(_bits(p_e), _bits(p_g)) and torch.equal(_bits(m_e), _bits(m_g))
    assert float(m_g.abs().max()) > 0


def _count_calls(L, names, log=None):
    calls = {n: 0 for n in names}
    saved = {n: getattr(L, n) for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            if log is not None:
                log.append((n, a))
            return saved[n](*a)
        return f
    for n in names:
        setattr(L, n, wrap(n))
    return calls, saved


def _instalments(runner):
    """The range lists ArenaOptimizerHook steps, by its own rule: early then late when the
    weight-gradient stream left a checkpoint in the step that just ran and there is an early part,
    else the merged ranges in one go."""
    early, late = runner.split_ranges()
    if runner.last_checkpoint is not None and early:
        return [early, late]
    return [runner.active_ranges]


def test_one_group_launch_per_instalment(hip_lib):
    """With groups: exactly one gs_sgd_step_groups launch per instalment (at most two per step) over
    that instalment's table, and at most one hyper write per step, whatever the fragment count; no
    gs_sgd_step.  Without paramwise_cfg: exactly the gs_sgd_step calls of the ungrouped path -- one
    per merged range of every instalment, in order, with the arena offsets, lengths, lr, momentum,
    weight decay, gradient scale and clear flag it has always passed -- and none of the new calls."""
    names = ("gs_sgd_step", "gs_sgd_step_hyper", "gs_sgd_set_hyper", "gs_sgd_step_groups",
             "gs_sgd_set_group_hyper")
    for grouped in (True, False):
        model = _model(fcn_head())
        opt = OPTIMIZER if grouped else {k: v for k, v in OPTIMIZER.items() if k != "paramwise_cfg"}
        runner, arena, pg = _runner(model, optimizer=opt)
        assert (pg is not None) == grouped and (arena.groups is not None) == grouped
        runner.call_hook("before_run")
        runner.set_arch(_anchor("sub"))
        runner.train_iter(_batch(0))          # (first step: module loading)
        per_step, log, split_seen = [], [], set()
        calls, saved = _count_calls(hip_lib, names, log)
        pb, gb, mb = arena.flat_param.data_ptr(), arena.flat_grad.data_ptr(), arena.flat_mom.data_ptr()
        try:
            for it, name in enumerate(["sub", "min", "max"], 1):
                before = dict(calls)
                del log[:]
                runner.set_arch(_anchor(name))
                runner.train_iter(_batch(it))
                per_step.append({n: calls[n] - before[n] for n in names})
                parts = _instalments(runner)
                split_seen.add(len(parts))
                st = log[-1][1][-1]            # (the stream every optimizer call of the step was given)
                if grouped:
                    nonempty = [r for r in parts if r]
                    assert sum(arena.chunk_table(r)[2] for r in nonempty) > 20          # fragments
                    want = [("gs_sgd_step_groups", (pb, gb, mb, arena.chunk_table(r)[0].data_ptr(),
                                                    arena.chunk_table(r)[1], arena.group_hyper.data_ptr(), 1, st))
                            for r in nonempty]
                    got = [c for c in log if c[0] != "gs_sgd_set_group_hyper"]
                    assert got == want and len(want) <= 2
                    assert per_step[-1]["gs_sgd_set_group_hyper"] <= 1
                else:
                    want = [("gs_sgd_step", (pb + 4 * a, gb + 4 * a, mb + 4 * a, b - a, runner.lr, 0.9, 5e-4,
                                             1.0, 1, st)) for r in parts for a, b in r]
                    assert log == want, (log, want)
                    if it >= 2:    # (past the two warm-up iterations: the poly lr, as always)
                        assert runner.lr == (0.01 - 1e-4) * (1 - it / 8) ** 0.9 + 1e-4
        finally:
            for n, f in saved.items():
                setattr(hip_lib, n, f)
        torch.cuda.synchronize()
        print("grouped=%s instalments seen %s, calls per step: %s" % (grouped, sorted(split_seen), per_step))


def test_graphs_keep_their_tables_through_cache_eviction(hip_lib):
    """A captured step graph names its chunk tables by address.  More than 512 other range sets go
    through the arena's table cache between the captures and the replays (as a long run with random
    subnets does): the anchors' entries are evicted and their memory would be free for the next
    upload, were it not owned by the graph entries.  The replays must still be bitwise the eager run."""
    names = ["sub", "min", "sub", "min", "sub", "sub", "min"]

    def run(graphs, churn_at=None):
        model = _model(fcn_head())
        runner, arena, _ = _runner(model)
        runner.graphs_enabled = graphs
        runner.call_hook("before_run")
        info = {}
        for it, name in enumerate(names):
            if it == churn_at:
                torch.cuda.synchronize()
                segs = [s for s in arena._tables.segs if s[2] >= 0][:40]
                held = [(k, v[0]) for k, v in arena._tables.entries.items()]
                for i in range(len(segs)):
                    for j in range(i, len(segs)):
                        if segs[j][1] - segs[i][0] == sum(e - b for b, e, _ in segs[i:j + 1]):   # contiguous
                            arena.chunk_table([(segs[i][0], segs[j][1])])
                info["evicted"] = sum(1 for k, _ in held if k not in arena._tables)
                info["kept"] = sum(len(e.keep) for e in runner._graphs.values())
                info["graphs"] = len(runner._graphs)
                torch.cuda.synchronize()
            runner.set_arch(_anchor(name))
            runner.train_iter(_batch(it))
        torch.cuda.synchronize()
        return arena.flat_param.clone(), arena.flat_mom.clone(), dict(runner.graph_stats), info

    p_e, m_e, _, _ = run(False)
    p_g, m_g, st, info = run(True, churn_at=4)
    assert st["captured"] == 2 and st["replayed"] >= 3, st
    # both graphs were live, owned a table and the hyper table per SGD launch, and every table of the
    # cache (theirs included) had been evicted before the last replays
    assert info["graphs"] == 2 and info["evicted"] >= 6 and info["kept"] >= 2 * 2, info
    assert torch.equal(_bits(p_e), _bits(p_g)) and torch.equal(_bits(m_e), _bits(m_g))


def test_sandwich_iteration_with_groups_matches_torch(hip_lib):
    """use_distillation with groups: the iteration's one union step equals torch's grouped SGD on the
    accumulated gradients (rel_err < 1e-6 per parameter)."""
    from gaia_seg_amd.core.model_space import build_model_sampler
    from gaia_seg_amd.core.runner import SandwichHook
    model = _model(psp_head(), seed=4)
    runner, arena, pg = _runner(model, hooks=False)
    sampler = build_model_sampler(dict(type="concat", model_samplers=[
        dict(type="anchor", anchors=[_anchor("max")]), dict(type="anchor", anchors=[_anchor("min")]),
        dict(type="anchor", anchors=[_anchor("sub")])]))
    sampler.seed(11)
    runner.register_hook(SandwichHook(sampler, dict(T=2.0, distillation_weight=0.5, interpolation=False)))
    twin = _TorchTwin(model, arena, pg)
    calls, saved = _count_calls(hip_lib, ("gs_sgd_step_groups", "gs_sgd_step"))
    try:
        runner.call_hook("before_run")
        for it in range(2):
            out = runner.train_iter(_batch(it))
            torch.cuda.synchronize()
            assert out["members"] == ["max", "min", "sub"] and len(twin.calls) == 1
            assert float(twin.calls[0][4].abs().max()) > 0          # the accumulated gradients
            twin.replay()
            name_w, err = twin.worst()
            print("sandwich iter %d: worst parameter %s rel_err %.3e" % (it, name_w, err))
            assert err < 1e-6, (name_w, err)
    finally:
        for n, f in saved.items():
            setattr(hip_lib, n, f)
    assert calls == {"gs_sgd_step_groups": 2, "gs_sgd_step": 0}
    assert arena.grads_clean and not arena.flat_grad.any() and not arena.flat_acc.any()


def test_train_supernet_cli_on_the_paramwise_config_through_resume(tmp_path):
    cfg = os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_paramwise.py")
    common = [sys.executable, os.path.join(ROOT, "tools", "train_supernet.py"), cfg, "--seed", "0",
              "--no-validate", "--cfg-options", "data.train.size=(128,256)", "log_config.interval=1",
              "checkpoint_config.interval=2"]
    first = os.path.join(str(tmp_path), "a")
    res = subprocess.run(common[:3] + ["--work-dir", first, "--max-iters", "2"] + common[3:],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    ck = os.path.join(first, "iter_2.pth")
    assert os.path.exists(ck)
    second = os.path.join(str(tmp_path), "b")
    res2 = subprocess.run(common[:3] + ["--work-dir", second, "--max-iters", "4", "--resume-from", ck]
                          + common[3:], capture_output=True, text=True, timeout=600)
    assert res2.returncode == 0, res2.stderr[-3000:]
    out = res2.stderr + res2.stdout
    assert "Iter [3/4]" in out and "Iter [4/4]" in out and "Iter [1/4]" not in out, out[-2000:]
    # the logged lr is group 0's: poly from 0.01 under the 500-iteration linear warm-up
    lr = float(re.search(r"Iter \[4/4\]\s+lr: ([0-9.e+-]+)", out).group(1))
    want = ((0.01 - 1e-4) * (1 - 3 / 4) ** 0.9 + 1e-4) * (1 - (1 - 3 / 500) * (1 - 1e-3))
    assert abs(lr - want) / want < 2e-3, (lr, want)
    a = torch.load(ck, map_location="cpu")
    b = torch.load(os.path.join(second, "iter_4.pth"), map_location="cpu")
    assert b["meta"]["iter"] == 4 and set(b["optimizer"]["state"]) == set(a["optimizer"]["state"])
    moved = [k for k in a["state_dict"] if a["state_dict"][k].is_floating_point()
             and not torch.equal(a["state_dict"][k], b["state_dict"][k])]
    assert any("decode_head" in k for k in moved) and any(k.startswith("backbone.layer") for k in moved)
    assert all(torch.isfinite(v).all() for v in b["state_dict"].values() if v.is_floating_point())
