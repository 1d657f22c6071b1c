"""DynamicASPPHead (DeepLabV3) and DynamicDepthwiseSeparableASPPHead (DeepLabV3+) on the GPU against the
float64 CPU restatement of tests/util_aspp.py: the tiny heads (channels 16, dilations (1, 2, 3, 5),
c1_channels 8) on an 8 x 12 feature map, N = 2, input widths sliced below the maxima.

TOL = 1e-3 is the project's parity bound (within 1e-3 rel of the CPU restatement)."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from util_aspp import head_cfg, load_into_ref, randomize_head, ref_head
from util_models import ARCHS, arch_meta, make_batch, model_cfg, randomize

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KINDS = pytest.mark.parametrize("separable", [False, True], ids=["v3", "v3plus"])


def make_inputs(n=2, seed=3, c=384, c1=64):
    """the four backbone levels of an OS8 network for a 64 x 96 image, stage widths below the tiny
    supernet's maxima (512 and 128): only levels 0 and 3 are read"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c1, 16, 24, generator=g), torch.randn(n, 8, 8, 12, generator=g),
            torch.randn(n, 8, 8, 12, generator=g), torch.randn(n, c, 8, 12, generator=g)]


def make_heads(separable, seed=0):
    from gaia_seg_amd.models import build_head
    prod = build_head(head_cfg(separable))
    randomize_head(prod, seed)
    ref = load_into_ref(ref_head(separable), prod).double()
    return prod.to(DEV), ref


@KINDS
def test_forward_backward_parity_in_training_mode(hip_lib, separable):
    """logits, input gradients, every head-parameter gradient and the BatchNorm running statistics"""
    prod, ref = make_heads(separable)
    prod.train()
    ref.train()
    inputs = make_inputs()
    used = (0, 3) if separable else (3,)
    xr = [t.double().requires_grad_(i in used) for i, t in enumerate(inputs)]
    xg = [t.to(DEV).requires_grad_(i in used) for i, t in enumerate(inputs)]
    want = ref(xr)
    gz = torch.randn(want.shape, generator=torch.Generator().manual_seed(5))
    want.backward(gz.double())
    got = prod(xg)
    got.backward(gz.to(DEV))
    errs = {"logits": rel_err(got, want)}
    for i in used:
        errs["d input %d" % i] = rel_err(xg[i].grad, xr[i].grad)
    ref_params = dict(ref.named_parameters())
    names = [k for k, _ in prod.named_parameters()]
    assert set(names) == set(ref_params) and len(names) > (40 if separable else 15)
    for k, p in prod.named_parameters():
        assert p.grad is not None, k
        assert float(ref_params[k].grad.abs().max()) > 0, k
        errs["d " + k] = rel_err(p.grad, ref_params[k].grad)
    ref_bufs = dict(ref.named_buffers())
    for k, b in prod.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            errs[k] = rel_err(b, ref_bufs[k])
    worst = max(errs, key=errs.get)
    print("%s: %d quantities, worst %s %.3g" % ("v3plus" if separable else "v3", len(errs), worst, errs[worst]))
    assert errs[worst] < TOL, {k: v for k, v in errs.items() if v >= TOL}
    if not separable:
        assert xg[0].grad is None        # DeepLabV3 reads inputs[in_index] only


@KINDS
def test_forward_parity_in_eval_mode(hip_lib, separable):
    prod, ref = make_heads(separable, seed=1)
    prod.eval()
    ref.eval()
    inputs = make_inputs(seed=4)
    before = {k: v.clone() for k, v in prod.state_dict().items()}
    with torch.no_grad():
        got = prod([t.to(DEV) for t in inputs])
        want = ref([t.double() for t in inputs])
    assert tuple(got.shape) == tuple(want.shape) == ((2, 19, 16, 24) if separable else (2, 19, 8, 12))
    err = rel_err(got, want)
    print("eval logits rel_err %.3g" % err)
    assert err < TOL
    for k, v in prod.state_dict().items():
        assert torch.equal(v, before[k]), k         # running statistics untouched


@KINDS
def test_concat_slices_equal_the_materialised_cat_bit_for_bit(hip_lib, separable):
    """Every branch writes into its slice of one buffer; the same branches written to buffers of their
    own and joined by torch.cat give the same bits (training mode: batch statistics)."""
    from gaia_seg_amd.hip import ops
    from gaia_seg_amd.hip.runtime import Act, Tape
    prod, _ = make_heads(separable, seed=2)
    prod.train()
    inputs = [t.to(DEV) for t in make_inputs(seed=6)]
    tape = Tape(enabled=False)
    with torch.no_grad():
        x = Act.from_nchw(inputs[3])
        fused = prod.aspp_concat(tape, x)
        pooled = ops.adaptive_avgpool(tape, x, [1])[0]
        pieces = [ops.bilinear(tape, prod.image_pool[1].forward_act(tape, pooled), (x.H, x.W), prod.align_corners)]
        pieces += [m.forward_act(tape, x) for m in prod.aspp_modules]
        torch.cuda.synchronize()
        assert fused.C == 5 * 16 and all(p.C == 16 for p in pieces)
        assert torch.equal(fused.t, torch.cat([p.t for p in pieces], dim=3))
        assert float(fused.t.abs().max()) > 0
        if separable:
            out = prod.bottleneck.forward_act(tape, fused)
            c1 = Act.from_nchw(inputs[0])
            fused2 = prod.c1_concat(tape, out, c1)
            pieces2 = [ops.bilinear(tape, out, (c1.H, c1.W), prod.align_corners),
                       prod.c1_bottleneck.forward_act(tape, c1)]
            torch.cuda.synchronize()
            assert (fused2.C, fused2.H, fused2.W) == (24, 16, 24)
            assert torch.equal(fused2.t, torch.cat([p.t for p in pieces2], dim=3))


@pytest.mark.parametrize("n,h,w,ci,co,dil", [(2, 8, 12, 32, 16, 12), (1, 40, 80, 16, 16, 36)],
                         ids=["dil12-on-8x12", "dil36-on-40x80"])
def test_dense_conv_bn_at_large_dilation(hip_lib, n, h, w, ci, co, dil):
    """The dense 3x3 ASPP branches: pad = dil as large as the map (every off-centre tap of most pixels
    in the padding) through ops.conv_bn, forward and backward, against float64.  Bounds: those of the
    operator's own test (tests/test_hip_ops_gpu.py::test_conv_bn_fused_calls), 1e-4 for the output
    and the running statistics and 2e-4 for the gradients; the second case is the configs' largest
    dilation, 36, on a map taller and wider than it."""
    from gaia_seg_amd.core.bricks import DynamicBatchNorm2d, DynamicConv2d, conv_bn_act, fused_call_ok
    from gaia_seg_amd.hip.runtime import tape_function
    torch.manual_seed(7)
    conv = DynamicConv2d(ci, co, 3, padding=dil, dilation=dil, bias=False)
    bn = DynamicBatchNorm2d(co)
    torch.nn.init.normal_(conv.weight, 0, 0.2)
    torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
    torch.nn.init.normal_(bn.bias, 0, 0.3)
    x = torch.randn(n, ci, h, w) + 0.5
    w_ref = conv.weight.detach().clone().contiguous().double().requires_grad_(True)
    g_ref = bn.weight.detach().clone().double().requires_grad_(True)
    b_ref = bn.bias.detach().clone().double().requires_grad_(True)
    x_ref = x.double().requires_grad_(True)
    rm, rv = torch.zeros(co, dtype=torch.float64), torch.ones(co, dtype=torch.float64)
    z_ref = F.relu(F.batch_norm(F.conv2d(x_ref, w_ref, None, 1, dil, dil), rm, rv, g_ref, b_ref, True, 0.1, 1e-5))
    gz = torch.randn(z_ref.shape)
    z_ref.backward(gz.double())
    conv, bn = conv.to(DEV), bn.to(DEV).train()
    assert fused_call_ok(conv, bn)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    z = tape_function(lambda tape, acts: [conv_bn_act(tape, conv, bn, acts[0], relu=True)], [xg], True)[0]
    z.backward(gz.to(DEV))
    errs = dict(z=rel_err(z, z_ref), mean=rel_err(bn.running_mean, rm), var=rel_err(bn.running_var, rv),
                dw=rel_err(conv.weight.grad, w_ref.grad), dgamma=rel_err(bn.weight.grad, g_ref.grad),
                dbeta=rel_err(bn.bias.grad, b_ref.grad), dx=rel_err(xg.grad, x_ref.grad))
    print(errs)
    assert max(errs[k] for k in ("z", "mean", "var")) < 1e-4, errs
    assert max(errs[k] for k in ("dw", "dgamma", "dbeta", "dx")) < 2e-4, errs


@KINDS
def test_one_image_in_training_raises_the_batchnorm_error(hip_lib, separable):
    prod, ref = make_heads(separable)
    prod.train()
    inputs = make_inputs(n=1)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        prod([t.to(DEV) for t in inputs])
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ref.train()([t.double() for t in inputs])


def test_depthwise_refuses_a_recording_tape_in_fp16_forward_precision_and_stays_fp32(hip_lib):
    from gaia_seg_amd.hip import ops
    prod, _ = make_heads(True, seed=1)
    dw = prod.sep_bottleneck[1].depthwise_conv.conv
    x = torch.randn(2, 16, 8, 12, device=DEV)
    with torch.no_grad():
        want = dw(x)
    with ops.forward_precision("fp16"):
        with pytest.raises(RuntimeError, match="fp16 forward precision is inference only"):
            dw(x.clone().requires_grad_(True))
        with torch.no_grad():
            assert torch.equal(dw(x), want)         # fp32 whatever the switch says
    with ops.train_precision("fp16"):
        with torch.no_grad():
            assert torch.equal(dw(x), want)


# ------------------------------------------------------------------------------------------
# the whole model: DeepLabV3+ with the auxiliary FCN head on the tiny OS8 supernet
# ------------------------------------------------------------------------------------------
def v3plus_cfg():
    return model_cfg(head_cfg(True), aux=True, os8=True)


def _runner(model, lr):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=lr,
                             momentum=0.9, weight_decay=1e-4, max_iters=100)
    runner.register_hook(ArenaOptimizerHook())
    return runner, arena


def _anchor(name):
    a = arch_meta(name)["backbone"]
    return {"name": name, "arch.backbone.stem.width": a["stem"]["width"],
            "arch.backbone.body.width": a["body"]["width"], "arch.backbone.body.depth": a["body"]["depth"]}


def test_step_graph_replay_equals_the_eager_step(hip_lib):
    """tests/test_runner_gpu.py's criterion on the DeepLabV3+ model: parameters, momentum, BatchNorm
    statistics and logged losses of replayed step graphs are bit-identical to eager steps."""
    from gaia_seg_amd.models import build_segmentor

    def run(graphs):
        torch.manual_seed(0)
        model = build_segmentor(copy.deepcopy(v3plus_cfg())).to(DEV).train()
        for h in (model.decode_head, model.auxiliary_head):
            h.dropout = None
        runner, arena = _runner(model, 0.05)
        runner.graphs_enabled = graphs
        runner.call_hook("before_run")
        logs = []
        for it, name in enumerate(["sub", "min", "sub", "min", "sub"]):
            runner.set_arch(_anchor(name))
            img, gt = make_batch(2, 64, 96, seed=it)
            metas = [dict(ori_shape=(64, 96, 3), img_shape=(64, 96, 3), flip=False) for _ in range(2)]
            out = runner.train_iter(dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV)))
            logs.append({k: float(v) for k, v in out["log_vars"].items()})
        torch.cuda.synchronize()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return sd, arena.flat_mom.detach().clone(), logs, dict(runner.graph_stats)

    sd_e, mom_e, logs_e, st_e = run(False)
    sd_g, mom_g, logs_g, st_g = run(True)
    assert st_e == {"captured": 0, "replayed": 0, "eager": 5}
    assert st_g["captured"] >= 1 and st_g["replayed"] >= 1, st_g
    assert logs_e == logs_g
    assert all(v == v for log in logs_e for v in log.values())
    assert torch.equal(mom_e, mom_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


def test_overfits_a_learnable_batch(hip_lib):
    """tests/test_model_gpu.py::test_overfits_a_learnable_batch on the DeepLabV3+ model: 60 steps on a
    fixed batch whose labels are a function of the image bring the loss below half the first."""
    from gaia_seg_amd.models import build_segmentor
    torch.manual_seed(0)
    model = build_segmentor(copy.deepcopy(v3plus_cfg())).to(DEV).train()
    model.manipulate_arch(arch_meta("sub"))
    runner, _ = _runner(model, 0.02)
    runner.set_arch(None)
    runner.call_hook("before_run")
    n, h, w = 2, 64, 96
    img = torch.randn(n, 3, h, w)
    sm = F.avg_pool2d(img[:, :1], 9, 1, 4)
    gt = ((sm - sm.min()) / (sm.max() - sm.min() + 1e-6) * 5.999).long()
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), flip=False) for _ in range(n)]
    batch = dict(img=img.to(DEV), img_metas=metas, gt_semantic_seg=gt.to(DEV))
    losses = []
    for _ in range(60):
        out = runner.train_iter(batch)
        losses.append(float(out["log_vars"]["decode.loss_seg"]))
    print(losses[::10], losses[-1])
    assert all(l == l for l in losses)
    assert losses[-1] < 0.5 * losses[0], losses[::10]


def test_extracted_subnet_equals_the_supernet_slice(hip_lib):
    """tools/extract_subnet.py's flow: the pruned copy has the subnet's shapes -- depthwise weights
    included -- and reproduces the supernet-slice logits."""
    from extract_subnet import extract
    from gaia_seg_amd.models import build_segmentor
    sup = build_segmentor(copy.deepcopy(v3plus_cfg()))
    randomize(sup)
    sup = sup.to(DEV).eval()
    n_sup = sum(p.numel() for p in sup.parameters())
    a = ARCHS["sub"]
    meta = {"name": "sub", "arch.backbone.stem.width": a["stem"],
            "arch.backbone.body.width": list(a["width"]), "arch.backbone.body.depth": list(a["depth"])}
    img, _ = make_batch(2, 64, 96)
    sup.manipulate_arch(arch_meta("sub"))
    with torch.no_grad():
        want = sup.encode_decode(img.to(DEV), None).clone()
    sup.deploy()
    sub = extract(sup, meta)
    sup.deploy(False)
    assert sum(p.numel() for p in sup.parameters()) == n_sup          # supernet untouched
    c4, c1 = 4 * a["width"][3], 4 * a["width"][0]
    head = sub.decode_head
    assert tuple(head.image_pool[1].conv.weight.shape) == (16, c4, 1, 1)
    assert tuple(head.aspp_modules[0].conv.weight.shape) == (16, c4, 1, 1)
    for m in list(head.aspp_modules)[1:]:
        dw = m.depthwise_conv
        assert tuple(dw.conv.weight.shape) == (c4, 1, 3, 3) and dw.conv.depthwise and dw.conv.groups == c4
        assert dw.bn.num_features == c4 and tuple(dw.bn.running_mean.shape) == (c4,)
        assert tuple(m.pointwise_conv.conv.weight.shape) == (16, c4, 1, 1)
    assert tuple(head.c1_bottleneck.conv.weight.shape) == (8, c1, 1, 1)
    assert tuple(head.sep_bottleneck[0].depthwise_conv.conv.weight.shape) == (24, 1, 3, 3)
    with torch.no_grad():
        got = sub.encode_decode(img.to(DEV), None)
    err = rel_err(got, want)
    print("extracted subnet rel_err %.3g" % err)
    assert err < 1e-6


def test_bn_calibrator_finds_the_new_batchnorm_layers(hip_lib):
    """BatchNorm re-calibration discovers layers by their bn_params calls: every BatchNorm of the
    DeepLabV3+ head is visited, the depthwise ones at the active input width."""
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.bricks import DynamicBatchNorm2d
    from gaia_seg_amd.models import build_segmentor
    model = build_segmentor(copy.deepcopy(v3plus_cfg())).to(DEV).eval()
    model.manipulate_arch(arch_meta("sub"))
    img, _ = make_batch(2, 64, 96)
    img = img.to(DEV)
    found = dict(BNCalibrator(model, [dict(img=img)])._discover(img))
    head_bns = {k: m for k, m in model.decode_head.named_modules() if isinstance(m, DynamicBatchNorm2d)}
    assert len(head_bns) == 2 + 7 + 1 + 4          # pool and bottleneck, ASPP, c1, sep_bottleneck
    for k, m in head_bns.items():
        assert m in found, k
    c4 = 4 * ARCHS["sub"]["width"][3]
    assert found[head_bns["aspp_modules.2.depthwise_conv.bn"]] == c4
    assert found[head_bns["sep_bottleneck.0.depthwise_conv.bn"]] == 24
    assert not any(m in found for m in model.auxiliary_head.modules())
