"""DynamicOCRHead behind a DynamicFCNHead in a DynamicCascadeEncoderDecoder on the GPU, after
tests/test_aspp_heads_gpu.py test for test and with its tolerances: the tiny cascade (FCN channels 16 on
stage 3, OCR channels 16 / ocr_channels 8 on stage 4) on the tiny OS8 / v1c backbone, a 32 x 48 input (4 x 6
feature maps: too small for BatchNorm trouble to hide), N = 2, dropout 0, against the float64 CPU
restatement of tests/util_ocr.py.

The parity tests hand the backbone's feature maps, computed once on the GPU, to both sides: the restatement
covers the two heads and the cascade flow (each stage's loss; stage 1 reading stage 0's logits with their
gradient), the backbone has its own oracle elsewhere.

TOL = 1e-3 is the project's parity bound (within 1e-3 rel of the CPU restatement)."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
import util_ocr as U
from util_models import ARCHS, arch_meta, make_batch, randomize

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
H, W = 32, 48
LOSS_KEYS = ["decode_0.acc_seg", "decode_0.loss_seg", "decode_1.acc_seg", "decode_1.loss_seg"]


def metas(n=2):
    return [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), flip=False) for _ in range(n)]


def make_pair(seed=0):
    """the product model on the GPU at the 'sub' arch, the float64 restatement of its two heads, and the
    backbone features of one batch (GPU tensors, and float64 CPU copies)"""
    from gaia_seg_amd.models import build_segmentor
    prod = build_segmentor(copy.deepcopy(U.cascade_cfg()))
    randomize(prod, seed)
    ref = U.ref_cascade()
    ref.decode_head.load_state_dict({k[len("decode_head."):]: v.detach().clone() for k, v in
                                     prod.state_dict().items() if k.startswith("decode_head.")}, strict=True)
    prod = prod.to(DEV)
    prod.manipulate_arch(arch_meta("sub"))
    img, gt = make_batch(2, H, W, seed=seed)
    prod.eval()
    with torch.no_grad():
        feats = [f.detach().clone() for f in prod.extract_feat(img.to(DEV))]
    torch.cuda.synchronize()
    assert tuple(feats[2].shape[2:]) == tuple(feats[3].shape[2:]) == (4, 6)
    return prod, ref.double(), feats, [f.cpu().double() for f in feats], gt


class LogitTap:
    """the logits every head hands to its ``losses`` (instance-level wrap, as tests/parity.py does)"""

    def __init__(self, heads):
        self.heads, self.logits = list(heads), []

    def __enter__(self):
        for h in self.heads:
            def tapped(seg_logit, seg_label, _orig=h.losses):
                self.logits.append(seg_logit.detach())
                return _orig(seg_logit, seg_label)
            h.__dict__["losses"] = tapped
        return self

    def __exit__(self, *exc):
        for h in self.heads:
            h.__dict__.pop("losses", None)
        return False


def hip_step(prod, feats, gt):
    """forward + backward of the cascade's training flow on given features: (losses, logits, feature grads)"""
    for p in prod.parameters():
        p.grad = None
    xs = [f.clone().requires_grad_(i in (2, 3)) for i, f in enumerate(feats)]
    with LogitTap(prod.decode_head) as tap:
        losses = prod._decode_head_forward_train(xs, metas(), gt.to(DEV))
    loss, _ = prod._parse_losses(losses)
    loss.backward()
    torch.cuda.synchronize()
    return losses, tap.logits, xs


def test_forward_backward_parity_in_training_mode(hip_lib):
    """losses, both heads' logits, the gradients of both feature maps, every head-parameter gradient -- the
    FCN head's included, which is the sum of its own loss and the path through the soft regions -- and the
    BatchNorm running statistics"""
    prod, ref, feats, feats_r, gt = make_pair()
    prod.train()
    ref.train()
    xr = [f.clone().requires_grad_(i in (2, 3)) for i, f in enumerate(feats_r)]
    losses_r, outs_r = ref.forward_train(xr, gt)
    (losses_r["decode_0.loss_seg"] + losses_r["decode_1.loss_seg"]).backward()
    losses, logits, xs = hip_step(prod, feats, gt)
    assert sorted(losses) == sorted(losses_r) == LOSS_KEYS
    errs = {}
    for k in LOSS_KEYS:
        got, want = float(losses[k]), float(losses_r[k])
        print("%s: %.6f (float64 %.6f)" % (k, got, want))
        if k.endswith("acc_seg"):       # a step function of the logits: two pixels may sit on a tie
            assert abs(got - want) / 100.0 * gt.numel() <= 2.01, k
        else:
            errs[k] = abs(got - want) / abs(want)
    assert len(logits) == 2
    for i in range(2):
        errs["logits %d" % i] = rel_err(logits[i], outs_r[i])
    for i in (2, 3):
        errs["d input %d" % i] = rel_err(xs[i].grad, xr[i].grad)
    assert xs[0].grad is None and xs[1].grad is None
    ref_params = dict(ref.named_parameters())
    names = [k for k, _ in prod.decode_head.named_parameters()]
    assert {"decode_head." + k for k in names} == set(ref_params) and len(names) == 5 + 26
    for k, p in prod.decode_head.named_parameters():
        want = ref_params["decode_head." + k].grad
        assert p.grad is not None, k
        assert float(want.abs().max()) > 0, k
        errs["d " + k] = rel_err(p.grad, want)
    ref_bufs = dict(ref.named_buffers())
    for k, b in prod.decode_head.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            errs[k] = rel_err(b, ref_bufs["decode_head." + k])
    worst = max(errs, key=errs.get)
    print("cascade: %d quantities, worst %s %.3g" % (len(errs), worst, errs[worst]))
    assert errs[worst] < TOL, {k: v for k, v in errs.items() if v >= TOL}
    # the path through the soft regions is really exercised: without decode_1's loss the FCN head's
    # gradients are other ones, and they are those of the restatement without that loss
    fcn_grads = {k: p.grad.detach().clone() for k, p in prod.decode_head[0].named_parameters()}
    prod.decode_head[1].loss_decode.loss_weight = 0.0
    hip_step(prod, feats, gt)
    ref0 = U.ref_cascade(ocr_loss_weight=0.0).double().train()
    ref0.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()}, strict=True)
    xr0 = [f.clone() for f in feats_r]
    losses_r0, _ = ref0.forward_train(xr0, gt)
    (losses_r0["decode_0.loss_seg"] + losses_r0["decode_1.loss_seg"]).backward()
    ref0_params = dict(ref0.named_parameters())
    for k, p in prod.decode_head[0].named_parameters():
        own = p.grad
        assert rel_err(own, ref0_params["decode_head.0." + k].grad) < TOL, k
        change = rel_err(fcn_grads[k], own)
        print("FCN %s: gradient changes by %.3g of its size with decode_1's loss" % (k, change))
        if k == "conv_seg.bias":
            # a constant added to a class map leaves its softmax over the pixels as it is: the classifier
            # bias gets nothing through the soft regions, in exact arithmetic
            assert change < TOL, k
        else:
            assert change > 10 * TOL, k
    for k, p in prod.decode_head[1].named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


def test_forward_parity_in_eval_mode(hip_lib):
    prod, ref, feats, feats_r, _ = make_pair(seed=1)
    prod.eval()
    ref.eval()
    before = {k: v.clone() for k, v in prod.state_dict().items()}
    with torch.no_grad():
        got = prod._decode_head_forward_test(feats, None)
        want = ref(feats_r)[-1]
    assert tuple(got.shape) == tuple(want.shape) == (2, 19, 4, 6)
    err = rel_err(got, want)
    print("eval logits rel_err %.3g" % err)
    assert err < TOL
    for k, v in prod.state_dict().items():
        assert torch.equal(v, before[k]), k         # running statistics untouched
    # the whole model's inference path goes through the same hook
    img, _ = make_batch(2, H, W, seed=1)
    with torch.no_grad():
        full = prod.encode_decode(img.to(DEV), None)
        labels = prod.simple_test_device(img.to(DEV), metas())
    assert tuple(full.shape) == (2, 19, H, W) and tuple(labels.shape) == (2, H, W)
    assert torch.equal(labels, full.argmax(dim=1))


def test_concat_slices_equal_the_materialised_cat_bit_for_bit(hip_lib):
    """The bottleneck and the output projection write into their halves of one buffer, and the gather and the
    query projection read the upper half at the buffer's pitch; the same pieces in buffers of their own,
    joined by torch.cat, give the same bits (training mode: batch statistics)."""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    prod, _, feats, _, _ = make_pair(seed=2)
    prod.train()
    head, ocb = prod.decode_head[1], prod.decode_head[1].object_context_block
    tape = Tape(enabled=False)
    with torch.no_grad():
        prev = Act.from_nchw(prod.decode_head[0].forward(feats))
        x = Act.from_nchw(feats[3])
        cat, fused_feats, fused_ctx = head.ocr_concat(tape, x, prev)
        fused_out = ocb.forward_acts(tape, cat, fused_feats, fused_ctx)
        f = head.bottleneck.forward_act(tape, x)
        ctx = ops.ocr_gather(tape, f, prev, 1.0)
        q = ocb.query_project[1].forward_act(tape, ocb.query_project[0].forward_act(tape, f))
        k = ocb.key_project[1].forward_act(tape, ocb.key_project[0].forward_act(tape, ctx))
        v = ocb.value_project.forward_act(tape, ctx)
        obj = ocb.out_project.forward_act(tape, ops.ocr_attend(tape, q, k, v))
        torch.cuda.synchronize()
        assert cat.C == 32 and obj.C == f.C == 16 and fused_feats.ld == 32 and f.ld == 16
        assert (ctx.N, ctx.H, ctx.W, ctx.C) == (2, 19, 1, 16)
        assert torch.equal(fused_ctx.t, ctx.t)
        assert torch.equal(cat.t, torch.cat([obj.t, f.t], dim=3))
        assert float(obj.t.abs().max()) > 0 and float(f.t.abs().max()) > 0
        assert torch.equal(fused_out.t, ocb.bottleneck.forward_act(tape, Act(torch.cat([obj.t, f.t], dim=3), False)).t)


def _runner(model, optimizer, max_iters=100):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.optimizer import build_param_groups, check_optimizer_cfg
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    opt = check_optimizer_cfg(optimizer)
    arena = ParamArena(model)
    if opt["type"] == "AdamW":
        arena.set_optimizer("AdamW", opt["betas"], opt["eps"])
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=opt["lr"],
                             momentum=opt.get("momentum", 0.0), weight_decay=opt["weight_decay"],
                             max_iters=max_iters, param_groups=build_param_groups(model, optimizer))
    runner.register_hook(ArenaOptimizerHook())
    return runner, arena


SGD = dict(type="SGD", lr=0.05, momentum=0.9, weight_decay=1e-4)
ADAMW = dict(type="AdamW", lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05)


def _anchor(name):
    a = arch_meta(name)["backbone"]
    return {"name": name, "arch.backbone.stem.width": a["stem"]["width"],
            "arch.backbone.body.width": a["body"]["width"], "arch.backbone.body.depth": a["body"]["depth"]}


def _batch(seed):
    img, gt = make_batch(2, H, W, seed=seed)
    return dict(img=img.to(DEV), img_metas=metas(), gt_semantic_seg=gt.to(DEV))


def test_step_graph_replay_equals_the_eager_step(hip_lib):
    """tests/test_runner_gpu.py's criterion on the cascade model: parameters, momentum, BatchNorm statistics
    and logged losses of replayed step graphs are bit-identical to eager steps."""
    from gaia_seg_amd.models import build_segmentor

    def run(graphs):
        torch.manual_seed(0)
        model = build_segmentor(copy.deepcopy(U.cascade_cfg())).to(DEV).train()
        runner, arena = _runner(model, SGD)
        runner.graphs_enabled = graphs
        runner.call_hook("before_run")
        logs = []
        for it, name in enumerate(["sub", "min", "sub", "min", "sub"]):
            runner.set_arch(_anchor(name))
            out = runner.train_iter(_batch(it))
            logs.append({k: float(v) for k, v in out["log_vars"].items()})
        torch.cuda.synchronize()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return sd, arena.flat_mom.detach().clone(), logs, dict(runner.graph_stats)

    sd_e, mom_e, logs_e, st_e = run(False)
    sd_g, mom_g, logs_g, st_g = run(True)
    assert st_e == {"captured": 0, "replayed": 0, "eager": 5}
    assert st_g["captured"] >= 1 and st_g["replayed"] >= 1, st_g
    assert logs_e == logs_g
    assert sorted(logs_e[0]) == sorted(LOSS_KEYS + ["loss"])
    assert all(v == v for log in logs_e for v in log.values())
    assert torch.equal(mom_e, mom_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


def test_overfits_a_learnable_batch(hip_lib):
    """tests/test_model_gpu.py::test_overfits_a_learnable_batch on the cascade model: 60 steps on a fixed
    batch whose labels are a function of the image bring both stages' losses below half the first."""
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(copy.deepcopy(U.cascade_cfg())).to(DEV).train()
    model.manipulate_arch(arch_meta("sub"))
    runner, _ = _runner(model, dict(SGD, lr=0.02))
    runner.set_arch(None)
    runner.call_hook("before_run")
    img = torch.randn(2, 3, H, W)
    sm = F.avg_pool2d(img[:, :1], 9, 1, 4)
    gt = ((sm - sm.min()) / (sm.max() - sm.min() + 1e-6) * 5.999).long()
    batch = dict(img=img.to(DEV), img_metas=metas(), gt_semantic_seg=gt.to(DEV))
    losses = []
    for _ in range(60):
        out = runner.train_iter(batch)
        losses.append((float(out["log_vars"]["decode_0.loss_seg"]), float(out["log_vars"]["decode_1.loss_seg"])))
    print(losses[::10], losses[-1])
    assert all(l == l for pair in losses for l in pair)
    assert losses[-1][1] < 0.5 * losses[0][1] and losses[-1][0] < 0.5 * losses[0][0], losses[::10]


def test_extracted_subnet_equals_the_supernet_slice(hip_lib):
    """tools/extract_subnet.py's flow: the pruned copy has the subnet's shapes in both heads and reproduces
    the supernet-slice logits."""
    from extract_subnet import extract
    from gaia_seg_amd.models import build_segmentor
    sup = build_segmentor(copy.deepcopy(U.cascade_cfg()))
    randomize(sup)
    sup = sup.to(DEV).eval()
    n_sup = sum(p.numel() for p in sup.parameters())
    a = ARCHS["sub"]
    meta = {"name": "sub", "arch.backbone.stem.width": a["stem"],
            "arch.backbone.body.width": list(a["width"]), "arch.backbone.body.depth": list(a["depth"])}
    img, _ = make_batch(2, H, W)
    sup.manipulate_arch(arch_meta("sub"))
    with torch.no_grad():
        want = sup.encode_decode(img.to(DEV), None).clone()
    sup.deploy()
    sub = extract(sup, meta)
    sup.deploy(False)
    assert sum(p.numel() for p in sup.parameters()) == n_sup          # supernet untouched
    c3, c4 = 4 * a["width"][2], 4 * a["width"][3]
    assert tuple(sub.decode_head[0].convs[0].conv.weight.shape) == (16, c3, 3, 3)
    assert tuple(sub.decode_head[1].bottleneck.conv.weight.shape) == (16, c4, 3, 3)
    assert tuple(sub.decode_head[1].object_context_block.query_project[0].conv.weight.shape) == (8, 16, 1, 1)
    with torch.no_grad():
        got = sub.encode_decode(img.to(DEV), None)
    err = rel_err(got, want)
    print("extracted subnet rel_err %.3g" % err)
    assert err < 1e-6


def test_bn_calibrator_finds_the_new_batchnorm_layers(hip_lib):
    """BatchNorm re-calibration discovers layers by their bn_params calls: every BatchNorm of both heads is
    visited, those on the region map included."""
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.bricks import DynamicBatchNorm2d
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(copy.deepcopy(U.cascade_cfg())).to(DEV).eval()
    model.manipulate_arch(arch_meta("sub"))
    img, _ = make_batch(2, H, W)
    img = img.to(DEV)
    found = dict(BNCalibrator(model, [dict(img=img)])._discover(img))
    head_bns = {k: m for k, m in model.decode_head.named_modules() if isinstance(m, DynamicBatchNorm2d)}
    assert len(head_bns) == 1 + 8          # the FCN conv; bottleneck, 2 query, 2 key, value, out, 1x1 bottleneck
    for k, m in head_bns.items():
        assert m in found, k
    assert found[head_bns["1.object_context_block.key_project.0.bn"]] == 8
    assert found[head_bns["1.bottleneck.bn"]] == 16


@pytest.mark.parametrize("optimizer", [SGD, ADAMW], ids=["sgd", "adamw"])
def test_one_training_step_through_the_runner(hip_lib, optimizer):
    """IterBasedRunner with the SGD and the AdamW optimizer: one step moves every active parameter of both
    heads and logs the four cascade losses"""
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(copy.deepcopy(U.cascade_cfg())).to(DEV).train()
    runner, arena = _runner(model, optimizer, max_iters=4)
    assert arena.optimizer == optimizer["type"]
    runner.call_hook("before_run")
    runner.set_arch(_anchor("sub"))
    before = {k: p.detach().clone() for k, p in model.decode_head.named_parameters()}
    out = runner.train_iter(_batch(0))
    torch.cuda.synchronize()
    assert sorted(out["log_vars"]) == sorted(LOSS_KEYS + ["loss"])
    assert all(float(v) == float(v) for v in out["log_vars"].values())
    for k, p in model.decode_head.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert not torch.equal(p, before[k]), "%s did not move" % k
