"""AdamW on the GPU: gs_adamw_step_groups against torch.optim.AdamW on the CPU (float32 twin for the
rel_err < 1e-6 comparisons, the same class on float64 copies where a margin is needed), per-parameter
step counters, untouched elements outside the table, and the runner on the tiny ViT and ConvNeXt
supernets (hook instalments with warm-up, step graphs, checkpoint / resume, fast-finetune restore, the
fp16 hook, an SGD runner that is what it was, the CLI)."""
import copy
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import util_convnext as UC
import util_vit as UV
from conftest import rel_err
from util_models import make_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

LR, WD, BETAS, EPS = 1e-2, 0.05, (0.9, 0.999), 1e-8
MULTS = [(1., 1.), (10., 1.), (1., 0.), (0., 1.)]
# (begin, end, group) in floats, tests/test_paramwise_gpu.py's layout: 128-float fragments, fragments that
# end off a chunk boundary (4096 / 16384), gaps that are in no chunk, the last fragment ending 64 floats
# before the arena's end.  Every fragment is one "parameter"; its step counter is slot 2 i + 1 of 20.
FRAGS = [(0, 128, 1), (128, 128 + 2 * 16384 + 192, 0), (33152, 33280, 2), (33280, 33408, 3),
         (33472, 38592, 0), (38592, 38720, 2), (38848, 38848 + 16384 + 64, 3), (55296, 59392 + 4, 1),
         (59456, 59456 + 4096, 2)]
PARAMS = [(b, e, g, 2 * i + 1) for i, (b, e, g) in enumerate(FRAGS)]
N_SLOTS = 20
ZERO_GRAD_PARAM = 5         # the (1, 0) parameter that is fed zero gradients
LEFT_OUT = (1, 6)           # parameters without a gradient in calls 2 and 4 (groups 0 and 3)
NUMEL = 59456 + 4096 + 64
UNUSED_SLOT = 77            # what the counters no parameter owns hold, before and after


def _stream():
    from gaia_seg_amd.hip.runtime import current_stream_ptr
    return current_stream_ptr()


def _set_hyper(L, hyper, lrs, wds, gscale=1.0, betas=BETAS, eps=EPS):
    from gaia_seg_amd.hip import lib
    g = lib.AdamwGroups()
    for i, (lr, wd) in enumerate(zip(lrs, wds)):
        g.lr_wd[2 * i], g.lr_wd[2 * i + 1] = lr, wd
    lib.check(L.gs_adamw_set_group_hyper(hyper.data_ptr(), betas[0], betas[1], eps, gscale, len(lrs), g,
                                         _stream()), "gs_adamw_set_group_hyper")


def _hyper():
    from gaia_seg_amd.hip import lib
    return torch.zeros(lib.ADAMW_HYPER_DOUBLES, dtype=torch.float64, device=DEV)


def _table(params, ch):
    from gaia_seg_amd.core.optimizer import chunk_table
    tab = chunk_table(params, ch)
    # bounds, on the host, before any launch: inside the arena, counters inside steps
    assert int((tab[:, 0].astype(np.int64) + tab[:, 1]).max()) * 4 <= NUMEL and tab[:, 0].min() >= 0
    assert 0 <= tab[:, 3].min() and tab[:, 3].max() < N_SLOTS
    return torch.from_numpy(tab).to(DEV), len(tab)


def _step(L, p, g, m, v, steps, table, n_chunks, hyper, zero):
    from gaia_seg_amd.hip import lib
    lib.check(L.gs_adamw_step_groups(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), steps.data_ptr(),
                                     steps.numel(), table.data_ptr(), n_chunks, hyper.data_ptr(), zero,
                                     _stream()), "gs_adamw_step_groups")


def _mask(params):
    m = torch.zeros(NUMEL, dtype=torch.bool)
    for b, e, *_ in params:
        m[b:e] = True
    return m


def _bits(t):
    return t.detach().cpu().view(torch.int32)


def _canary(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (NUMEL,), generator=g, dtype=torch.int64).to(torch.int32)


def _twin(p0, dtype=torch.float32, lrs=None, wds=None, state=None):
    """torch.optim.AdamW on CPU copies, one tensor and one param group per parameter of PARAMS"""
    lrs = lrs if lrs is not None else [LR * lm for lm, _ in MULTS]
    wds = wds if wds is not None else [WD * dm for _, dm in MULTS]
    ref = [p0[b:e].to(dtype).clone().requires_grad_(True) for b, e, _, _ in PARAMS]
    opt = torch.optim.AdamW([dict(params=[ref[i]], lr=lrs[g], weight_decay=wds[g])
                             for i, (_, _, g, _) in enumerate(PARAMS)], lr=LR, betas=BETAS, eps=EPS,
                            weight_decay=WD)
    if state is not None:
        t, m0, v0 = state
        for i, (b, e, _, _) in enumerate(PARAMS):
            opt.state[ref[i]] = dict(step=torch.tensor(float(t)), exp_avg=m0[b:e].to(dtype).clone(),
                                     exp_avg_sq=v0[b:e].to(dtype).clone())
    return ref, opt


@pytest.mark.parametrize("ch", [4096, 16384])
def test_adamw_matches_torch_with_per_parameter_steps(hip_lib, ch):
    """Five calls, zero_grad alternating, four groups (1,1) (10,1) (1,0) (0,1), two parameters without a
    gradient in calls 2 and 4: parameters and both moments at rel_err < 1e-6 of torch.optim.AdamW (the
    SGD operator tests' bound), counters equal to torch's state['step'], nothing outside the table
    touched in any of the four arenas."""
    from gaia_seg_amd.core.optimizer import chunk_table
    torch.manual_seed(0)
    lrs = [LR * lm for lm, _ in MULTS]
    wds = [WD * dm for _, dm in MULTS]
    full = _table(PARAMS, ch)
    part = _table([q for i, q in enumerate(PARAMS) if i not in LEFT_OUT], ch)
    assert full[1] > len(PARAMS) and part[1] < full[1]
    inside = _mask(PARAMS)
    inside_part = _mask([q for i, q in enumerate(PARAMS) if i not in LEFT_OUT])
    zb, ze = PARAMS[ZERO_GRAD_PARAM][:2]
    # canaries outside the table in all four arenas (NaN patterns included), zero moments inside
    p0 = torch.randn(NUMEL)
    p0.view(torch.int32)[~inside] = _canary(1)[~inside]
    m0, v0 = torch.zeros(NUMEL), torch.zeros(NUMEL)
    m0.view(torch.int32)[~inside] = _canary(2)[~inside]
    v0.view(torch.int32)[~inside] = _canary(3)[~inside]
    ref, opt = _twin(torch.where(inside, p0, torch.zeros(())))
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    steps0 = torch.full((N_SLOTS,), UNUSED_SLOT, dtype=torch.int32)
    for *_, slot in PARAMS:
        steps0[slot] = 0
    steps = steps0.to(DEV)
    hyper = _hyper()
    _set_hyper(hip_lib, hyper, lrs, wds)
    for call in range(5):
        g = torch.randn(NUMEL)
        g[zb:ze] = 0.
        g.view(torch.int32)[~inside] = _canary(10 + call)[~inside]
        partial = call in (1, 3)
        for i, (b, e, _, _) in enumerate(PARAMS):
            ref[i].grad = None if partial and i in LEFT_OUT else g[b:e].clone()
        opt.step()
        gg = g.to(DEV)
        zero = call % 2
        table, n_chunks = part if partial else full
        _step(hip_lib, p, gg, m, v, steps, table, n_chunks, hyper, zero)
        torch.cuda.synchronize()
        covered = inside_part if partial else inside
        if zero:       # cleared inside THIS call's table, bitwise untouched outside it
            assert float(gg.cpu()[covered].abs().max()) == 0.0
            assert torch.equal(_bits(gg)[~covered], _bits(g)[~covered])
        else:
            assert torch.equal(_bits(gg), _bits(g))
    pc, mc, vc, sc = p.cpu(), m.cpu(), v.cpu(), steps.cpu()
    for i, (b, e, grp, slot) in enumerate(PARAMS):
        st = opt.state[ref[i]]
        errs = (rel_err(pc[b:e], ref[i]), rel_err(mc[b:e], st["exp_avg"]), rel_err(vc[b:e], st["exp_avg_sq"]))
        print("ch %d parameter %d group %s: rel_err p %.3e m %.3e v %.3e, step %d"
              % (ch, i, MULTS[grp], *errs, int(sc[slot])))
        assert max(errs) < 1e-6, (i, errs)
        assert int(sc[slot]) == int(st["step"]) == (3 if i in LEFT_OUT else 5)
    for slot in set(range(N_SLOTS)) - {q[3] for q in PARAMS}:
        assert int(sc[slot]) == UNUSED_SLOT
    for i, (b, e, grp, _) in enumerate(PARAMS):
        if grp == 3:       # lr_mult 0: parameters bitwise alone while both moments move
            assert torch.equal(_bits(pc)[b:e], _bits(p0)[b:e])
            assert float(mc[b:e].abs().min()) > 0 and float(vc[b:e].min()) > 0
    assert torch.equal(_bits(pc)[zb:ze], _bits(p0)[zb:ze])          # (1, 0) with zero gradients
    assert float(mc[zb:ze].abs().max()) == 0.0 and float(vc[zb:ze].abs().max()) == 0.0
    b2, e2 = PARAMS[2][:2]
    assert not torch.equal(pc[b2:e2], p0[b2:e2])                    # the other (1, 0) parameter moved
    for name, t, t0 in (("param", pc, p0), ("exp_avg", mc, m0), ("exp_avg_sq", vc, v0)):
        assert torch.equal(_bits(t)[~inside], _bits(t0)[~inside]), name
    # the hyper table holds the doubles it was given, not their float roundings
    h = hyper.cpu().tolist()
    assert h[:5] == [BETAS[0], BETAS[1], EPS, 1.0, 4.0] and h[8:16] == [x for pr in zip(lrs, wds) for x in pr]
    # an entry naming a group the hyper table lacks or a slot outside steps is skipped, counters included
    _set_hyper(hip_lib, hyper, lrs[:2], wds[:2])
    before = [t.clone() for t in (p, m, v, steps)]
    gg = torch.randn(NUMEL, device=DEV)
    g_before = gg.clone()
    bad = [q for q in PARAMS if q[2] >= 2] + [(PARAMS[0][0], PARAMS[0][1], 0, N_SLOTS)]
    tab = torch.from_numpy(chunk_table(bad, ch)).to(DEV)
    _step(hip_lib, p, gg, m, v, steps, tab, len(tab), hyper, 1)
    torch.cuda.synchronize()
    for t, t0 in zip((p, m, v, steps, gg), before + [g_before]):
        assert torch.equal(t.cpu().view(torch.int32), t0.cpu().view(torch.int32))


def test_first_step_is_within_2e6_of_float64_elementwise(hip_lib):
    """p0 = 0, zero state, |g| log-uniform in [1e-3, 1], betas (0.9, 0.999), lr 1e-2: every element of p1
    within 2e-6 relative of torch.optim.AdamW on float64 copies.  The chain g*gscale -> m -> v -> sqrt ->
    /sqrt(bc2) -> +eps -> lr/bc1 -> divide has about ten fp32 roundings of 6e-8 each; 2e-6 is that with a
    threefold margin.  A float beta2 (1 - beta2 off by 1.3e-5) or an fp32 1 - powf bias correction
    (about 3e-5 at t = 1) fails it.  Measured on the MI355X: worst element 3.2e-7 (profiles/r16_adamw.md)."""
    g0 = torch.Generator().manual_seed(5)
    mag = 10.0 ** (-3.0 * torch.rand(NUMEL, generator=g0, dtype=torch.float64))
    sign = torch.where(torch.rand(NUMEL, generator=g0) < 0.5, -1.0, 1.0).double()
    g = (mag * sign).float()
    assert 1e-3 <= float(g.abs().min()) and float(g.abs().max()) <= 1.0
    params = [(b, e, 0, s) for b, e, _, s in PARAMS]
    table, n_chunks = _table(params, 4096)
    ref, opt = _twin(torch.zeros(NUMEL), torch.float64, lrs=[LR] * 4, wds=[WD] * 4)
    for i, (b, e, _, _) in enumerate(PARAMS):
        ref[i].grad = g[b:e].double()
    opt.step()
    p, m, v = (torch.zeros(NUMEL, device=DEV) for _ in range(3))
    steps = torch.zeros(N_SLOTS, dtype=torch.int32, device=DEV)
    hyper = _hyper()
    _set_hyper(hip_lib, hyper, [LR], [WD])
    _step(hip_lib, p, g.to(DEV), m, v, steps, table, n_chunks, hyper, 0)
    torch.cuda.synchronize()
    pc, worst = p.cpu().double(), 0.0
    for i, (b, e, _, _) in enumerate(PARAMS):
        want = ref[i].detach()
        assert float(want.abs().min()) > 0.3 * LR                  # every element moved by about lr
        worst = max(worst, float(((pc[b:e] - want).abs() / want.abs()).max()))
    print("first step: worst element %.3e relative to the float64 twin" % worst)
    assert worst <= 2e-6, worst
    assert steps.cpu()[[q[3] for q in PARAMS]].tolist() == [1] * len(PARAMS) and int(steps.sum()) == len(PARAMS)


@pytest.mark.parametrize("t0", [1000, 100000])
def test_bias_corrections_far_from_the_first_step(hip_lib, t0):
    """Counters preset to t0 (and the twin's state['step'] with them): two more calls stay at
    rel_err < 1e-6 of torch.optim.AdamW, counters end at t0 + 2."""
    torch.manual_seed(t0)
    inside = _mask(PARAMS)
    p0 = torch.where(inside, torch.randn(NUMEL), torch.zeros(()))
    m0 = torch.where(inside, torch.randn(NUMEL) * 0.1, torch.zeros(()))
    v0 = torch.where(inside, torch.rand(NUMEL) * 0.5 + 1e-3, torch.zeros(()))
    ref, opt = _twin(p0, state=(t0, m0, v0))
    table, n_chunks = _table(PARAMS, 4096)
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    steps = torch.full((N_SLOTS,), t0, dtype=torch.int32, device=DEV)
    hyper = _hyper()
    _set_hyper(hip_lib, hyper, [LR * lm for lm, _ in MULTS], [WD * dm for _, dm in MULTS])
    for call in range(2):
        g = torch.randn(NUMEL)
        for i, (b, e, _, _) in enumerate(PARAMS):
            ref[i].grad = g[b:e].clone()
        opt.step()
        _step(hip_lib, p, g.to(DEV), m, v, steps, table, n_chunks, hyper, call)
    torch.cuda.synchronize()
    pc, mc, vc, sc = p.cpu(), m.cpu(), v.cpu(), steps.cpu()
    for i, (b, e, grp, slot) in enumerate(PARAMS):
        st = opt.state[ref[i]]
        errs = (rel_err(pc[b:e], ref[i]), rel_err(mc[b:e], st["exp_avg"]), rel_err(vc[b:e], st["exp_avg_sq"]))
        print("t0 %d parameter %d: rel_err p %.3e m %.3e v %.3e" % (t0, i, *errs))
        assert max(errs) < 1e-6, (i, errs)
        assert int(sc[slot]) == int(st["step"]) == t0 + 2
        assert grp == 3 or not torch.equal(pc[b:e], p0[b:e])


# ---- the runner ----
PARAMWISE = dict(custom_keys={"pos_embed": dict(decay_mult=0.), "cls_token": dict(decay_mult=0.)},
                 norm_decay_mult=0.)
OPTIMIZER = dict(type="AdamW", lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05, paramwise_cfg=PARAMWISE)
LR_CONFIG = dict(power=1.0, min_lr=0.0, by_epoch=False, warmup="linear", warmup_iters=2, warmup_ratio=1e-3)
FAMILIES = {"vit": (UV, UV.randomize_vit, UV.TINY["img_size"]), "convnext": (UC, UC.randomize_convnext, (64, 96))}


def _model(family, seed=0):
    from gaia_seg_amd.models import build_segmentor
    U, randomize, _ = FAMILIES[family]
    torch.manual_seed(seed)
    model = build_segmentor(copy.deepcopy(U.tiny_model_cfg()))
    randomize(model.backbone, seed)
    for h in (model.decode_head, model.auxiliary_head):
        h.dropout = None
    return model.to(DEV).train()


def _batch(family, seed):
    h, w = FAMILIES[family][2]
    img, gt = make_batch(2, h, w, seed=seed)
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(h, w, 3), flip=False) for _ in range(2)]
    return dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))


def _meta(family, name):
    return FAMILIES[family][0].arch_meta(name)


def _runner(model, optimizer=OPTIMIZER, lr_config=LR_CONFIG, max_iters=8, hook=None):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner, PolyLrUpdaterHook
    opt = check_optimizer_cfg(optimizer)
    arena = ParamArena(model)
    if opt["type"] == "AdamW":
        arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    pg = build_param_groups(model, optimizer)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=opt.get("momentum", 0.0), weight_decay=opt["weight_decay"],
                             max_iters=max_iters, param_groups=pg)
    runner.register_hook(PolyLrUpdaterHook(**lr_config))
    runner.register_hook(hook if hook is not None else ArenaOptimizerHook())
    return runner, arena, pg


class _AdamTwin:
    """torch.optim.AdamW on CPU copies of the arena segments, one param group per parameter group, stepped
    with the gradients and per-group lr / weight decay the arena's adamw_step was given."""

    def __init__(self, model, arena, pg):
        self.arena, self.pg = arena, pg
        flat = arena.flat_param.detach().cpu()
        self.params, self.seg, self.slot = {}, {}, {}
        for i, (name, p) in enumerate(model.named_parameters()):
            o, n = arena.segments[id(p)]
            self.seg[name], self.slot[name] = (o, n), i
            self.params[name] = flat[o:o + n].clone().requires_grad_(True)
        groups = [dict(params=[self.params[n] for n in pg.members(g)], lr=0.0, weight_decay=0.0)
                  for g in range(len(pg))]
        self.opt = torch.optim.AdamW([g for g in groups if g["params"]], lr=0.0, betas=arena.betas, eps=arena.eps)
        self.group_of = {id(self.params[n]): g for n, g in pg.index.items()}
        self.calls = []
        orig = arena.adamw_step

        def recorded(ranges, lr, weight_decay, grad_scale=1.0, zero_grad=False, hyper=None):
            self.calls.append((list(ranges), list(lr), list(weight_decay), grad_scale,
                               arena.flat_grad.detach().cpu().clone()))
            return orig(ranges, lr, weight_decay, grad_scale, zero_grad, hyper=hyper)
        arena.adamw_step = recorded

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
        """worst rel_err over parameters, exp_avg, exp_avg_sq; and the counters, which must be equal"""
        a = self.arena
        flat, mom, var = (t.detach().cpu() for t in (a.flat_param, a.flat_mom, a.flat_var))
        steps = a.steps.cpu().tolist()
        worst, counts = ("", 0.0), {}
        for name, (o, k) in self.seg.items():
            st = self.opt.state.get(self.params[name])
            errs = [rel_err(flat[o:o + k], self.params[name])]
            if st:
                errs += [rel_err(mom[o:o + k], st["exp_avg"]), rel_err(var[o:o + k], st["exp_avg_sq"])]
                assert steps[self.slot[name]] == int(st["step"]), name
            else:      # never stepped: no state in torch, zero state and counter here
                assert steps[self.slot[name]] == 0 and not mom[o:o + k].any() and not var[o:o + k].any(), name
            counts[name] = steps[self.slot[name]]
            if max(errs) > worst[1]:
                worst = (name, max(errs))
        return worst, counts


@pytest.mark.parametrize("family", ["vit", "convnext"])
def test_runner_steps_equal_torch_adamw(hip_lib, family):
    """Four iterations alternating a depth-skipping subnet and the max one, paramwise_cfg as in the AdamW
    configs, two-iteration linear warm-up, through ArenaOptimizerHook: every parameter and both moments at
    rel_err < 1e-6 of torch.optim.AdamW fed the same gradients and per-group lr after each iteration; the
    blocks 'sub' skips are stepped twice, the rest four times, and the counters equal torch's."""
    model = _model(family)
    runner, arena, pg = _runner(model)
    assert pg.groups == [(1., 1.), (1., 0.)] and arena.groups == 2 and arena.optimizer == "AdamW"
    assert {n for n in pg.members(1) if "pos_embed" in n or "cls_token" in n} or family != "vit"
    twin = _AdamTwin(model, arena, pg)
    runner.call_hook("before_run")
    for it, name in enumerate(["sub", "max", "sub", "max"]):
        runner.set_arch(_meta(family, name))
        runner.train_iter(_batch(family, it))
        torch.cuda.synchronize()
        assert twin.calls and all(c[1] == runner.group_lr for c in twin.calls)
        assert all(c[2] == [0.05, 0.0] for c in twin.calls)
        twin.replay()
        (name_w, err), counts = twin.worst()
        print("%s iter %d (%s): worst %s rel_err %.3e, group lr %s" % (family, it, name, name_w, err, runner.group_lr))
        assert err < 1e-6, (it, name_w, err)
        assert arena.grads_clean and not arena.flat_grad.any()
    # warm-up over iterations 0 and 1, then the linear schedule
    assert runner.group_lr == pytest.approx([1e-3 * (1 - 3 / 8)] * 2, rel=1e-12)
    trained = {n: c for n, c in counts.items() if n in pg.index}
    assert set(trained.values()) >= {2, 4} and set(trained.values()) <= {0, 2, 4}, set(trained.values())
    skipped = [n for n, c in trained.items() if c == 2]
    assert skipped and all(n.startswith("backbone.") for n in skipped)
    assert float(arena.flat_var.max()) > 0


def _run_iters(family, names, graphs=False, stop_after=None, resume=None, tmp=None, optimizer=OPTIMIZER):
    """a fresh model and runner over ``names`` (from iteration len(resumed)); -> arena state"""
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    model = _model(family)
    runner, arena, _ = _runner(model, optimizer=optimizer)
    runner.graphs_enabled = graphs
    if resume is not None:
        runner.resume(resume)
    runner.call_hook("before_run")
    for it in range(runner.iter, len(names)):
        runner.set_arch(_meta(family, names[it]))
        runner.train_iter(_batch(family, it))
        if stop_after is not None and it + 1 == stop_after:
            torch.cuda.synchronize()
            save_checkpoint(model, tmp, optimizer=arena, meta=dict(iter=it + 1))
            break
    torch.cuda.synchronize()
    state = dict(p=arena.flat_param.clone(), m=arena.flat_mom.clone(), steps=arena.steps.clone() if
                 arena.steps is not None else None, v=arena.flat_var.clone() if arena.flat_var is not None else None)
    return state, dict(runner.graph_stats), model, arena


def _same_state(a, b):
    for k in ("p", "m", "v"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert torch.equal(a["steps"], b["steps"])


def test_step_graph_replay_is_bitwise_the_eager_run(hip_lib):
    names = ["sub", "max", "sub", "max", "sub", "sub", "max"]
    eager, st_e, _, _ = _run_iters("vit", names)
    graph, st_g, _, _ = _run_iters("vit", names, graphs=True)
    assert st_e["replayed"] == 0 and st_e["captured"] == 0
    assert st_g["replayed"] > 0 and st_g["captured"] == 2, st_g
    _same_state(eager, graph)
    assert float(graph["v"].max()) > 0 and int(graph["steps"].max()) == 7 and 0 < int(graph["steps"][graph["steps"] > 0].min()) < 7


def test_checkpoint_resume_is_bitwise_the_uninterrupted_run(hip_lib, tmp_path):
    names = ["sub", "max", "sub", "max", "sub"]
    whole, _, _, _ = _run_iters("convnext", names)
    ck = str(tmp_path / "iter_3.pth")
    _run_iters("convnext", names, stop_after=3, tmp=ck)
    saved = torch.load(ck, map_location="cpu")["optimizer"]
    assert saved["format"] == "gaia_seg_amd.adamw.v1" and tuple(saved["betas"]) == (0.9, 0.999) and saved["eps"] == 1e-8
    ent = saved["state"]["backbone.stem.weight"]
    assert set(ent) == {"step", "exp_avg", "exp_avg_sq"} and ent["step"] == 3
    assert tuple(ent["exp_avg"].shape) == (8, 3, 4, 4)                     # logical OIHW
    assert {e["step"] for e in saved["state"].values()} >= {1, 3}
    resumed, _, _, _ = _run_iters("convnext", names, resume=ck)
    _same_state(whole, resumed)


def test_foreign_optimizer_state_restarts_from_zero(hip_lib):
    from gaia_seg_amd.core.param_arena import ParamArena
    adam, _, _, arena_a = _run_iters("convnext", ["sub", "max"])
    sgd_opt = dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4)
    sgd, _, _, arena_s = _run_iters("convnext", ["sub", "max"], optimizer=sgd_opt)
    assert sgd["v"] is None and sgd["steps"] is None and arena_s.flat_var is None
    sd_a, sd_s = arena_a.state_dict(), arena_s.state_dict()
    assert sd_s["format"] == "gaia_seg_amd.sgd_momentum.v1" and float(arena_a.flat_mom.abs().max()) > 0
    # SGD momentum is never loaded as exp_avg: the AdamW arena warns and restarts from zero
    with pytest.warns(UserWarning, match="foreign format"):
        assert arena_a.load_state_dict(sd_s) is False
    assert not arena_a.flat_mom.any() and not arena_a.flat_var.any() and not arena_a.steps.any()
    # its own format comes back bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert arena_a.load_state_dict(sd_a) is True
    assert torch.equal(_bits(arena_a.flat_mom), _bits(adam["m"])) and torch.equal(arena_a.steps, adam["steps"])
    assert torch.equal(_bits(arena_a.flat_var), _bits(adam["v"]))
    # the converse: AdamW state into a fresh SGD arena leaves its momentum zero
    fresh = ParamArena(_model("convnext"))
    with pytest.warns(UserWarning, match="foreign format"):
        assert fresh.load_state_dict(sd_a) is False
    assert not fresh.flat_mom.any() and fresh.flat_var is None


def test_finetune_restore_resets_adamw_state_and_rows_do_not_depend_on_order(hip_lib):
    from gaia_seg_amd.apis import finetune as ft
    from gaia_seg_amd.core.config import Config
    cfg = Config(dict(optimizer=dict(OPTIMIZER, paramwise_cfg=dict(norm_decay_mult=0.)), optimizer_config=dict(),
                      lr_config=dict(policy="poly", power=1.0, min_lr=0.0, by_epoch=False),
                      runner=dict(type="IterBasedRunner", max_iters=2), data=dict(samples_per_gpu=2)))
    A = dict(_meta("convnext", "sub"), name="A")
    B = dict(_meta("convnext", "max"), name="B")

    def run(metas):
        model = _model("convnext", seed=3)
        inside, made = {}, []
        real = ft.prepare_training
        ft.prepare_training = lambda m, c: made.append(real(m, c)) or made[-1]
        try:
            rows = ft.finetune_model_space(
                model, metas, cfg, [_batch("convnext", s) for s in (3, 4)], [_batch("convnext", 11)], 1,
                on_subnet=lambda row, m: inside.__setitem__(
                    row["name"], {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
        finally:
            ft.prepare_training = real
        torch.cuda.synchronize()
        return {r["name"]: r for r in rows}, inside, made[0][1]

    rows_ab, in_ab, arena = run([A, B])
    assert arena.optimizer == "AdamW"
    # the restore behind the last subnet: both moments and every counter zero
    assert not arena.flat_mom.any() and not arena.flat_var.any() and not arena.steps.any()
    rows_ba, in_ba, _ = run([B, A])
    for name in ("A", "B"):
        assert rows_ab[name] == rows_ba[name], name
        assert all(torch.equal(in_ab[name][k], in_ba[name][k]) for k in in_ab[name]), name
    # restore() on an arena that has stepped
    state, _, model, arena = _run_iters("convnext", ["sub", "max"])
    assert arena.flat_var.any() and arena.steps.any()
    snap = ft.SupernetSnapshot(model, arena)
    snap.restore()
    assert not arena.flat_mom.any() and not arena.flat_var.any() and not arena.steps.any() and arena.grads_clean


def test_fp16_hook_feeds_adamw_the_unscaled_gradient(hip_lib):
    """Fp16OptimizerHook(loss_scale=512) on AdamW: the one update equals the twin fed grad / 512."""
    from gaia_seg_amd.core.runner import Fp16ArenaOptimizerHook
    model = _model("convnext")
    runner, arena, pg = _runner(model, hook=Fp16ArenaOptimizerHook(loss_scale=512.))
    twin = _AdamTwin(model, arena, pg)
    runner.call_hook("before_run")
    runner.set_arch(_meta("convnext", "max"))
    runner.train_iter(_batch("convnext", 0))
    torch.cuda.synchronize()
    assert twin.calls and all(c[3] == 1.0 / 512 for c in twin.calls)
    assert float(max(c[4].abs().max() for c in twin.calls)) > 0
    twin.replay()
    (name_w, err), counts = twin.worst()
    print("fp16 hook: worst %s rel_err %.3e" % (name_w, err))
    assert err < 1e-6 and max(counts.values()) == 1


def _count_calls(L, names):
    calls = {n: 0 for n in names}
    saved = {n: getattr(L, n) for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            return saved[n](*a)
        return f
    for n in names:
        setattr(L, n, wrap(n))
    return calls, saved


def test_an_sgd_runner_is_what_it_was(hip_lib):
    """SGD: no second moment, no counters, and the optimizer entry points of one iteration are the ones
    the runner has always called -- gs_sgd_step per merged range without groups, one gs_sgd_step_groups
    per instalment with them -- and never a gs_adamw_* call.  An AdamW runner makes no gs_sgd_* call."""
    names = ("gs_sgd_step", "gs_sgd_step_hyper", "gs_sgd_set_hyper", "gs_sgd_step_groups",
             "gs_sgd_set_group_hyper", "gs_adamw_step_groups", "gs_adamw_set_group_hyper")
    sgd = dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=5e-4)
    for opt in (sgd, dict(sgd, paramwise_cfg=dict(norm_decay_mult=0.)), OPTIMIZER):
        model = _model("convnext")
        runner, arena, pg = _runner(model, optimizer=opt)
        runner.call_hook("before_run")
        runner.set_arch(_meta("convnext", "sub"))
        runner.train_iter(_batch("convnext", 0))          # (first step: module loading)
        calls, saved = _count_calls(hip_lib, names)
        try:
            runner.train_iter(_batch("convnext", 1))
        finally:
            for n, f in saved.items():
                setattr(hip_lib, n, f)
        torch.cuda.synchronize()
        early, late = runner.split_ranges()
        parts = [early, late] if runner.last_checkpoint is not None and early else [runner.active_ranges]
        parts = [r for r in parts if r]
        print("%s paramwise=%s: %s" % (opt["type"], "paramwise_cfg" in opt, calls))
        if opt["type"] == "SGD":
            assert arena.flat_var is None and arena.steps is None and arena.adamw_hyper is None
            assert calls["gs_adamw_step_groups"] == 0 and calls["gs_adamw_set_group_hyper"] == 0
            assert calls["gs_sgd_step_hyper"] == 0 and calls["gs_sgd_set_hyper"] == 0
            if pg is None:
                assert calls["gs_sgd_step"] == sum(len(r) for r in parts) and calls["gs_sgd_step_groups"] == 0
                assert calls["gs_sgd_set_group_hyper"] == 0
            else:
                assert calls["gs_sgd_step_groups"] == len(parts) and calls["gs_sgd_step"] == 0
                assert calls["gs_sgd_set_group_hyper"] <= 1
        else:
            assert calls["gs_adamw_step_groups"] == len(parts) and calls["gs_adamw_set_group_hyper"] <= 1
            assert all(calls[n] == 0 for n in names if n.startswith("gs_sgd"))


def test_train_supernet_cli_writes_an_adamw_checkpoint(tmp_path):
    cfg_path = tmp_path / "tiny_adamw.py"
    anchors = [UC.arch_meta("max"), UC.arch_meta("sub")]
    cfg_path.write_text(
        "model = %r\n"
        "train_sampler = dict(type='anchor', anchors=%r)\n"
        "val_sampler = dict(type='anchor', anchors=%r)\n"
        "data = dict(samples_per_gpu=2, workers_per_gpu=2,\n"
        "            train=dict(type='SyntheticSegDataset', size=(64, 96), num_classes=19))\n"
        "optimizer = %r\n"
        "optimizer_config = dict()\n"
        "lr_config = dict(policy='poly', power=1.0, min_lr=0.0, by_epoch=False, warmup='linear',\n"
        "                 warmup_iters=2, warmup_ratio=1e-3)\n"
        "runner = dict(type='IterBasedRunner', max_iters=3)\n"
        "checkpoint_config = dict(by_epoch=False, interval=3)\n"
        "log_config = dict(interval=1)\n"
        % (UC.tiny_model_cfg(), anchors, anchors, dict(OPTIMIZER, paramwise_cfg=dict(norm_decay_mult=0.))))
    work = tmp_path / "w"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_supernet.py"), str(cfg_path),
                          "--work-dir", str(work), "--seed", "0", "--no-validate"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert "Iter [3/3]" in res.stdout + res.stderr
    ck = torch.load(str(work / "iter_3.pth"), map_location="cpu")
    opt = ck["optimizer"]
    assert opt["format"] == "gaia_seg_amd.adamw.v1" and ck["meta"]["iter"] == 3
    steps = {e["step"] for e in opt["state"].values()}
    assert max(steps) == 3 and all(torch.isfinite(e["exp_avg_sq"]).all() for e in opt["state"].values())
    assert any(float(e["exp_avg_sq"].max()) > 0 for e in opt["state"].values())
