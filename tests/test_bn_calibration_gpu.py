"""Per-subnet BatchNorm re-calibration on one MI355X: the fold kernel bit for bit, the calibrated
statistics against the CPU oracle's cumulative average, and the promise that the supernet is
bit-identical after every use (ranking, fp16, elastic input, the training hook, the CLI)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from parity import TOL
from util_models import arch_meta, fcn_head, make_batch, make_pair, model_cfg, psp_head

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, H, W = 3, 2, 64, 96


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _calib_batches(k=K):
    return [dict(img=make_batch(N, H, W, seed=20 + i)[0].cuda(),
                 img_metas=[dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), flip=False) for _ in range(N)])
            for i in range(k)]


def _val_batch(seed):
    img, gt = make_batch(N, H, W, seed=seed)
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), flip=False) for _ in range(N)]
    return dict(img=img.cuda(), img_metas=metas, gt_semantic_seg=gt.cuda())


def _anchor(name):
    a = arch_meta(name)["backbone"]
    return {"name": name, "arch.backbone.stem.width": a["stem"]["width"],
            "arch.backbone.body.width": a["body"]["width"], "arch.backbone.body.depth": a["body"]["depth"]}


def _model(head=None, arch="sub", seed=0):
    prod, _ = make_pair(model_cfg(head or fcn_head(), aux=True), seed=seed)
    prod = prod.cuda().eval()
    prod.manipulate_arch(arch_meta(arch))
    return prod


def _raw_state(model):
    """Parameters, buffers (NOT through state_dict(): that folds the host-side batch counters) and the
    host-side state a calibration touches."""
    from torch.nn.modules.batchnorm import _BatchNorm
    torch.cuda.synchronize()
    tensors = {"p:" + k: v.detach().clone() for k, v in model.named_parameters()}
    tensors.update({"b:" + k: v.detach().clone() for k, v in model.named_buffers()})
    host = {k: (m.training, getattr(m, "momentum", None), getattr(m, "sync", None),
                m.__dict__.get("_nbt_pending")) if isinstance(m, _BatchNorm) else (m.training,)
            for k, m in model.named_modules()}
    return tensors, host


def _assert_same_state(model, state):
    tensors, host = state
    now_t, now_h = _raw_state(model)
    assert now_t.keys() == tensors.keys()
    for k, v in tensors.items():
        assert torch.equal(now_t[k], v), k
    assert now_h == host


def _bn_stats(model):
    return {k: v.detach().clone() for k, v in model.named_buffers()
            if k.endswith(("running_mean", "running_var"))}


# ------------------------------------------------------------------------------------------------
# 1. the kernel, exact
# ------------------------------------------------------------------------------------------------
SENT = -777.25       # beyond a buffer's active slice
BANK_SENT = 555.5    # bank floats outside the layers' ranges


def _device_table(lib, entries):
    host = (lib.BnCalibLayer * len(entries))()
    for e, (rm, rv, c, off) in zip(host, entries):
        e.running_mean, e.running_var, e.channels, e.offset = rm, rv, c, off
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fold_kernel_matches_numpy_bit_for_bit(hip_lib):
    from gaia_seg_amd.hip import lib
    rng = np.random.RandomState(0)
    chans, sizes, offs = (4, 20, 7, 0), (8, 32, 16, 4), (2, 12, 54, 70)
    bank_floats = 80   # ranges [2,10) [12,52) [54,68) and an empty one at 70

    def fresh():
        out = []
        for c, n in zip(chans, sizes):
            pair = []
            for lo in (0.0, 0.5):   # mean-like and variance-like values
                a = np.full(n, SENT, np.float32)
                a[:c] = (rng.randn(c) * 3 + lo).astype(np.float32)
                pair.append(a)
            out.append(pair)
        return out

    host = fresh()
    dev = [[torch.from_numpy(a.copy()).cuda() for a in pair] for pair in host]
    table = _device_table(lib, [(m.data_ptr(), v.data_ptr(), c, o)
                                for (m, v), c, o in zip(dev, chans, offs)])

    def upload(vals):
        for (m, v), (hm, hv) in zip(dev, vals):
            m.copy_(torch.from_numpy(hm))
            v.copy_(torch.from_numpy(hv))

    def fold(bank, op, scale=1.0, tab=table, n=len(chans), floats=bank_floats):
        assert hip_lib.gs_bn_calib_fold(tab.data_ptr(), n, bank.data_ptr(), floats, op, scale, None) == 0

    covered = np.zeros(bank_floats, bool)
    for c, o in zip(chans, offs):
        covered[o:o + 2 * c] = True
    save = torch.full((bank_floats,), BANK_SENT, device="cuda")
    acc_host = np.full(bank_floats, BANK_SENT, np.float32)
    acc_host[covered] = 0.0     # the accumulator is zeroed before the first ADD
    acc = torch.from_numpy(acc_host.copy()).cuda()

    fold(save, lib.BN_CALIB_SAVE)
    want_save = np.full(bank_floats, BANK_SENT, np.float32)
    for (hm, hv), c, o in zip(host, chans, offs):
        want_save[o:o + c], want_save[o + c:o + 2 * c] = hm[:c], hv[:c]
    assert np.array_equal(_bits(save.cpu().numpy()), _bits(want_save))

    want_acc = acc_host.copy()
    for _ in range(3):
        vals = fresh()
        upload(vals)
        fold(acc, lib.BN_CALIB_ADD)
        for (hm, hv), c, o in zip(vals, chans, offs):
            want_acc[o:o + c] = want_acc[o:o + c] + hm[:c]
            want_acc[o + c:o + 2 * c] = want_acc[o + c:o + 2 * c] + hv[:c]
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want_acc))

    third = np.float32(1.0 / 3.0)
    fold(acc, lib.BN_CALIB_WRITE, 1.0 / 3.0)
    for (m, v), c, n, o in zip(dev, chans, sizes, offs):
        for t, lo in ((m, o), (v, o + c)):
            want = np.full(n, SENT, np.float32)
            want[:c] = want_acc[lo:lo + c] * third
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want_acc))    # WRITE reads the bank only

    fold(save, lib.BN_CALIB_WRITE, 1.0)
    for (m, v), (hm, hv) in zip(dev, host):
        assert np.array_equal(_bits(m.cpu().numpy()), _bits(hm))
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(hv))

    # entries that do not fit are skipped, their neighbours are processed.  (The bank handed over is a
    # window of a larger allocation, so an entry that were followed would still land in owned memory.)
    big = torch.full((256,), BANK_SENT, device="cuda")
    bank = big[64:64 + 32]
    (m0, v0), (m1, v1), (m2, v2) = dev[0], dev[1], dev[2]
    tab2 = _device_table(lib, [(m0.data_ptr(), v0.data_ptr(), 4, 0),       # fits: [0, 8)
                               (m1.data_ptr(), v1.data_ptr(), 20, 8),      # 8 + 40 > 32
                               (m1.data_ptr(), v1.data_ptr(), -1, 8),      # negative channels
                               (m1.data_ptr(), v1.data_ptr(), 4, -8),      # negative offset
                               (m1.data_ptr(), v1.data_ptr(), 4, 28),      # 28 + 8 > 32
                               (m2.data_ptr(), v2.data_ptr(), 7, 18)])     # fits exactly: [18, 32)
    fold(bank, lib.BN_CALIB_SAVE, tab=tab2, n=6, floats=32)
    want = np.full(256, BANK_SENT, np.float32)
    want[64:68], want[68:72] = host[0][0][:4], host[0][1][:4]
    want[64 + 18:64 + 25], want[64 + 25:64 + 32] = host[2][0][:7], host[2][1][:7]
    assert np.array_equal(_bits(big.cpu().numpy()), _bits(want))
    # ... and WRITE through the same table leaves the skipped layer's buffers alone
    big.mul_(2.0)
    fold(bank, lib.BN_CALIB_WRITE, 1.0, tab=tab2, n=6, floats=32)
    assert np.array_equal(_bits(m1.cpu().numpy()), _bits(host[1][0]))
    assert np.array_equal(_bits(v1.cpu().numpy()), _bits(host[1][1]))
    assert np.array_equal(_bits(m0.cpu().numpy()[:4]), _bits(host[0][0][:4] * np.float32(2)))
    assert float(m0[4]) == SENT and float(v2[7]) == SENT

    # argument errors, before any launch
    t, b = table.data_ptr(), save.data_ptr()
    assert hip_lib.gs_bn_calib_fold(None, 4, b, bank_floats, 0, 1.0, None) == -4
    assert hip_lib.gs_bn_calib_fold(t, 4, None, bank_floats, 0, 1.0, None) == -4
    assert hip_lib.gs_bn_calib_fold(t, 0, b, bank_floats, 0, 1.0, None) == -1
    assert hip_lib.gs_bn_calib_fold(t, 4, b, 0, 0, 1.0, None) == -1
    assert hip_lib.gs_bn_calib_fold(t, 4, b, bank_floats, 3, 1.0, None) == -1
    assert hip_lib.gs_bn_calib_fold(t, 4, b, bank_floats, -1, 1.0, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(_bits(save.cpu().numpy()), _bits(want_save))


# ------------------------------------------------------------------------------------------------
# 2. against the oracle: the cumulative average of K batches' statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["fcn", "psp"])
def test_calibrated_statistics_match_the_oracle(hip_lib, head):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from oracle.model import OBN
    cfg = model_cfg(fcn_head() if head == "fcn" else psp_head(), aux=True)
    prod, orc = make_pair(cfg)
    prod = prod.cuda().eval()
    meta = arch_meta("sub")
    prod.manipulate_arch(meta)
    orc.manipulate_arch(meta)
    batches = _calib_batches()

    orc.double().train()
    before_o = {k: v.detach().clone() for k, v in orc.named_buffers()}
    with torch.no_grad():
        for k, b in enumerate(batches, 1):
            for m in orc.modules():
                if isinstance(m, OBN):
                    m.momentum = 1.0 / k      # the cumulative average (momentum=None after a reset)
            orc.decode_head(orc.backbone(b["img"].cpu().double()))
    after_o = dict(orc.named_buffers())

    before = _bn_stats(prod)
    state = _raw_state(prod)
    with BNCalibrator(prod, batches).calibrated():
        torch.cuda.synchronize()
        inside = _bn_stats(prod)
        assert not prod.training
    _assert_same_state(prod, state)

    visited, worst = 0, (0.0, None)
    for name, got in inside.items():
        moved = (after_o[name] != before_o[name]).cuda()      # the slices the oracle's forward wrote
        # what the subnet does not read is untouched bit for bit: channels beyond the active slice,
        # the auxiliary head, depth-skipped blocks
        assert torch.equal(got[~moved], before[name][~moved]), name
        if not bool(moved.any()):
            continue
        assert not name.startswith("auxiliary_head"), name
        visited += 1
        e = rel_err(got[moved], after_o[name][moved.cpu()])
        worst = max(worst, (e, name))
        assert e < TOL, (name, e)
    print("%s: %d visited layers, worst %.3e at %s" % (head, visited // 2, worst[0], worst[1]))
    assert visited // 2 > 15
    # 'sub' runs 2 of the 3 blocks of stage 3: the third block and the auxiliary head were compared
    # bit for bit above, and nothing of them moved on the oracle either
    assert not any(bool((after_o[k] != before_o[k]).any()) for k in after_o
                   if k.startswith(("backbone.layer3.2.", "auxiliary_head.")) and "running" in k)


# ------------------------------------------------------------------------------------------------
# 3. restore
# ------------------------------------------------------------------------------------------------
def _runner(model, max_iters=100):
    from gaia_seg_amd.core.dist import GradReducer
    from gaia_seg_amd.core.param_arena import ParamArena
    from gaia_seg_amd.core.runner import ArenaOptimizerHook, IterBasedRunner
    arena = ParamArena(model)
    runner = IterBasedRunner(model, arena, GradReducer(arena.flat_grad, arena.segments), base_lr=0.05,
                             momentum=0.9, weight_decay=5e-4, max_iters=max_iters)
    runner.register_hook(ArenaOptimizerHook())
    return runner, arena


def test_supernet_is_bit_identical_after_the_block(hip_lib):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    models = [_model().train() for _ in range(2)]
    runners = [_runner(m) for m in models]
    for (r, _), m in zip(runners, models):
        r.set_arch(_anchor("sub"))
        r.train_iter(_val_batch(1))          # pending host-side batch counts, non-trivial momentum
    a, b = models
    cal = BNCalibrator(a, _calib_batches())
    state = _raw_state(a)
    assert any(h[3] for h in state[1].values() if len(h) == 4), "no pending batch count to preserve"
    assert a.training
    with cal.calibrated():
        assert not a.training
        inside = _bn_stats(a)
    _assert_same_state(a, state)
    assert any(not torch.equal(inside[k], state[0]["b:" + k]) for k in inside)

    # through state_dict() as well, num_batches_tracked included
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    with cal.calibrated():
        pass
    sd2 = a.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert int(sd["backbone.bn1.num_batches_tracked"]) == 1

    # an exception inside the block still restores
    state = _raw_state(a)
    with pytest.raises(RuntimeError, match="inside"):
        with cal.calibrated():
            raise RuntimeError("inside")
    _assert_same_state(a, state)

    # the next training step equals the one of a model that was never calibrated
    b.state_dict()      # (the counters of b are folded as a's were above)
    for r, _ in runners:
        r.train_iter(_val_batch(2))
    torch.cuda.synchronize()
    assert torch.equal(runners[0][1].flat_param, runners[1][1].flat_param)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------
# 4. / 5. ranking
# ------------------------------------------------------------------------------------------------
METRICS = ("mIoU", "mAcc", "aAcc")


def test_calibrated_rows_do_not_depend_on_the_order(hip_lib):
    from gaia_seg_amd.apis.test import test_model_space
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    model = _model()
    cal = BNCalibrator(model, _calib_batches())
    loader = [_val_batch(7), _val_batch(8)]
    A, B = _anchor("min"), _anchor("sub")
    state = _raw_state(model)
    ab = test_model_space(model, loader, [A, B], 2, 19, metric_tag="calibrated", calibrator=cal)
    ba = test_model_space(model, loader, [B, A], 2, 19, metric_tag="calibrated", calibrator=cal)
    _assert_same_state(model, state)
    assert [r["name"] for r in ab] == ["min", "sub"] and [r["name"] for r in ba] == ["sub", "min"]
    assert ab[0] == ba[1] and ab[1] == ba[0]


def test_default_rows_unchanged_and_calibrated_rows_differ(hip_lib):
    from gaia_seg_amd.apis.test import test_model_space
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.evaluation import evaluate_model
    model = _model()      # util_models.randomize: running statistics that belong to no subnet
    loader = [_val_batch(7), _val_batch(8)]
    metas = [_anchor("min"), _anchor("sub"), _anchor("max")]
    direct = test_model_space(model, loader, metas, 2, 19)
    for meta, row in zip(metas, direct):
        model.manipulate_arch(arch_meta(meta["name"]))
        res = evaluate_model(model, loader, 2, 19)
        assert all(row["metric.direct.%s" % k] == res[k] for k in METRICS), meta["name"]
    calibrated = test_model_space(model, loader, metas, 2, 19, metric_tag="calibrated",
                                  calibrator=BNCalibrator(model, _calib_batches()))
    for d, c in zip(direct, calibrated):
        assert all(0.0 <= c["metric.calibrated.%s" % k] <= 1.0 for k in METRICS)
        assert tuple(c["metric.calibrated.%s" % k] for k in METRICS) != \
            tuple(d["metric.direct.%s" % k] for k in METRICS), d["name"]
    # and the direct rows are what they were
    assert test_model_space(model, loader, metas, 2, 19) == direct


# ------------------------------------------------------------------------------------------------
# 6. fp16   7. input shape
# ------------------------------------------------------------------------------------------------
def test_fp16_calibration_runs_the_f16_loop_and_restores(hip_lib):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.fp16_utils import wrap_fp16_model
    model = _model(arch="max")
    cal32 = BNCalibrator(model, _calib_batches())
    with cal32.calibrated():
        stats32 = _bn_stats(model)
    wrap_fp16_model(model)
    state = _raw_state(model)
    n, f = ctypes.c_int64(), ctypes.c_double()
    hip_lib.gs_debug_f16_launches(ctypes.byref(n), ctypes.byref(f), 1)
    with BNCalibrator(model, _calib_batches()).calibrated():
        hip_lib.gs_debug_f16_launches(ctypes.byref(n), ctypes.byref(f), 1)
        stats16 = _bn_stats(model)
    assert n.value > 0, "the calibration forwards did not reach the fp16 loop"
    assert hip_lib.gs_get_forward_precision() == 0
    _assert_same_state(model, state)
    # fp16 operands: not equal to the fp32 calibration, and close to it -- an operand rounding of 2^-11
    # per conv, growing at worst linearly over the ~30 convs of the MAX subnet: 30 * 2 * 2^-11 = 3e-2
    assert any(not torch.equal(stats16[k], stats32[k]) for k in stats16)
    assert all(rel_err(stats16[k], stats32[k]) < 0.05 for k in stats16)


def test_calibration_at_an_input_shape(hip_lib):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    model = _model()
    cal = BNCalibrator(model, _calib_batches())
    state = _raw_state(model)
    with cal.calibrated():
        full = _bn_stats(model)
    with cal.calibrated(input_shape=48):       # short side 48: 48 x 72
        small = _bn_stats(model)
    with cal.calibrated(input_shape=64):       # the batches' own size: the same statistics
        same = _bn_stats(model)
    _assert_same_state(model, state)
    assert any(not torch.equal(full[k], small[k]) for k in full)
    assert all(torch.equal(full[k], same[k]) for k in full)
    assert all(torch.equal(b["img"], c["img"]) for b, c in zip(cal.batches, _calib_batches()))


# ------------------------------------------------------------------------------------------------
# 8. the training hook
# ------------------------------------------------------------------------------------------------
def test_eval_hook_with_calibrator_leaves_the_run_bit_identical(hip_lib):
    from gaia_seg_amd.core.bn_calibration import BNCalibrator
    from gaia_seg_amd.core.evaluation import CrossArchEvalHook
    from gaia_seg_amd.core.model_space import build_model_sampler
    finals, results = [], []
    for interval in (2, 100):
        model = _model().train()
        runner, arena = _runner(model, max_iters=4)
        sampler = build_model_sampler(dict(type="anchor", anchors=[_anchor("min"), _anchor("max")]))
        hook = CrossArchEvalHook([_val_batch(5)], sampler, interval=interval, num_batches=1,
                                 calibrator=BNCalibrator(model, _calib_batches()))
        runner.register_hook(hook)
        runner.set_arch(_anchor("sub"))
        runner.run([[_val_batch(i) for i in range(4)]])
        torch.cuda.synchronize()
        assert runner.iter == 4 and model.training and runner.arch_name == "sub"
        finals.append((arena.flat_param.clone(), {k: v.clone() for k, v in model.state_dict().items()}))
        results.append(hook.results)
    assert [it for it, _ in results[0]] == [2, 4] and results[1] == []
    assert all(0.0 <= r["mIoU"] <= 1.0 for _, out in results[0] for r in out.values())
    (pa, sa), (pb, sb) = finals
    assert torch.equal(pa, pb)
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------
# 9. the CLI
# ------------------------------------------------------------------------------------------------
CLI_CFG = """
model = %(model)r
train_cfg = dict()
test_cfg = dict(mode='whole')
data = dict(samples_per_gpu=2, workers_per_gpu=1, train=dict(type='SyntheticSegDataset', size=(64, 96)))
evaluation = dict(interval=8000, metric='mIoU', num_batches=2)
caliberate_bn = dict(recalibrate=dict(num_batches=3, seed=4))
"""


def test_cli_writes_calibrated_rows(hip_lib, tmp_path):
    from gaia_seg_amd.apis.test import test_model_space
    from gaia_seg_amd.apis.train import build_dataloader
    from gaia_seg_amd.core.bn_calibration import BNCalibrator, build_calibration_batches
    from gaia_seg_amd.core.checkpoint import save_checkpoint
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.model_space import dump_model_space
    mc = model_cfg(fcn_head(), aux=True)
    cfg_path = tmp_path / "tiny_calibrated.py"
    cfg_path.write_text(CLI_CFG % dict(model={k: v for k, v in mc.items() if k not in ("train_cfg", "test_cfg")}))
    prod, _ = make_pair(mc)
    ck = str(tmp_path / "supernet.pth")
    save_checkpoint(prod, ck)
    space = str(tmp_path / "space.json")
    metas = [_anchor("min"), _anchor("sub")]
    dump_model_space(metas, space)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test_supernet.py"), str(cfg_path), ck,
                          "--model-space-path", space, "--work-dir", str(tmp_path), "--seed", "0",
                          "--metric-tag", "calibrated"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    rows = json.load(open(tmp_path / "test_supernet" / "metrics.json"))
    assert [r["name"] for r in rows] == ["min", "sub"]
    assert all("metric.calibrated.%s" % k in r for r in rows for k in METRICS)
    assert not any(k.startswith("metric.direct") for r in rows for k in r)

    # the same rows in process: the tool's val batches, the config's calibration batches
    cfg = Config.fromfile(str(cfg_path))
    model = prod.cuda().eval()
    it = iter(build_dataloader(cfg.data["train"], 2, seed=12345, device="cuda", num_classes=19))
    loader = [next(it) for _ in range(2)]
    cal = BNCalibrator(model, build_calibration_batches(cfg, device="cuda"))
    here = test_model_space(model, loader, metas, 2, 19, metric_tag="calibrated", calibrator=cal)
    direct = test_model_space(model, loader, metas, 2, 19)
    for r, h, d in zip(rows, here, direct):
        assert all(r["metric.calibrated.%s" % k] == h["metric.calibrated.%s" % k] for k in METRICS), r["name"]
        assert tuple(h["metric.calibrated.%s" % k] for k in METRICS) != \
            tuple(d["metric.direct.%s" % k] for k in METRICS)
