"""tools/test_supernet.py end to end on one MI355X: a checkpoint from the training CLI, a model
space from tools/count_flops.py, the example rules config, fp32 and fp16 runs, and a follow-up
'top' rule over the written metrics file."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "supernet", "fcn_ar50to101v2_test_supernet.py")
SMALL = ["data.train.size=(128,256)", "data.samples_per_gpu=1", "evaluation.num_batches=2"]


def _run(cmd, timeout):
    res = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res


def test_test_supernet_cli_end_to_end(tmp_path):
    from gaia_seg_amd.core.model_space import ModelSpace
    tr = tmp_path / "train"
    _run([os.path.join(ROOT, "tools", "train_supernet.py"), os.path.join(ROOT, "configs", "supernet",
          "fcn_ar50to101v2.py"), "--work-dir", str(tr), "--seed", "0", "--no-validate", "--max-iters", "2",
          "--cfg-options", "data.train.size=(128,256)", "log_config.interval=1", "checkpoint_config.interval=2"],
         600)
    ck = str(tr / "iter_2.pth")
    space = str(tmp_path / "flops.json")
    _run([os.path.join(ROOT, "tools", "count_flops.py"), CFG, "--out", space], 300)
    rows_in = ModelSpace.load(space).rows
    assert [r["name"] for r in rows_in] == ["R50", "R77", "R101"]
    wd = tmp_path / "work"
    tool = os.path.join(ROOT, "tools", "test_supernet.py")
    _run([tool, CFG, ck, "--model-space-path", space, "--work-dir", str(wd), "--seed", "0",
          "--cfg-options"] + SMALL, 600)
    out32 = wd / "test_supernet" / "metrics.json"
    rows32 = json.load(open(out32))
    assert sorted(r["name"] for r in rows32) == ["R101", "R50", "R77"]
    for r in rows32:
        for k in ("mIoU", "mAcc", "aAcc"):
            assert math.isfinite(r["metric.direct.%s" % k]) and 0.0 <= r["metric.direct.%s" % k] <= 1.0
        assert r["overhead.flops"] == next(x for x in rows_in if x["name"] == r["name"])["overhead.flops"]

    # fp32 rows equal a direct evaluate_model call per subnet (same checkpoint, same batches)
    from gaia_seg_amd.apis.train import build_dataloader
    from gaia_seg_amd.core.checkpoint import load_checkpoint
    from gaia_seg_amd.core.config import Config
    from gaia_seg_amd.core.dynamic import fold_dict
    from gaia_seg_amd.core.evaluation import evaluate_model
    from gaia_seg_amd.models import build_segmentor
    cfg = Config.fromfile(CFG)
    cfg.merge_from_dict({"data.train.size": (128, 256), "data.samples_per_gpu": 1})
    model = build_segmentor(cfg.model, train_cfg=cfg.get("train_cfg"), test_cfg=cfg.get("test_cfg"))
    load_checkpoint(model, ck, strict=False)
    model = model.cuda().eval()
    loader = build_dataloader(cfg.data["train"], 1, seed=12345, device="cuda", num_classes=19)
    it = iter(loader)
    batches = [next(it) for _ in range(2)]
    for r in rows32:
        model.manipulate_arch(fold_dict(dict((k, list(v) if isinstance(v, list) else v)
                                             for k, v in r.items()))["arch"])
        res = evaluate_model(model, batches, 2, 19)
        assert res["mIoU"] == r["metric.direct.mIoU"] and res["aAcc"] == r["metric.direct.aAcc"], r["name"]
        assert res["mAcc"] == r["metric.direct.mAcc"], r["name"]
    del model
    torch.cuda.empty_cache()

    # fp16 run over the written file: its own tag, the fp32 columns kept
    _run([tool, CFG, ck, "--model-space-path", str(out32), "--work-dir", str(wd), "--seed", "0",
          "--metric-tag", "fp16", "--out-name", "metrics_fp16.json",
          "--cfg-options", "fp16.loss_scale=512.0"] + SMALL, 600)
    rows16 = json.load(open(wd / "test_supernet" / "metrics_fp16.json"))
    by32 = {r["name"]: r for r in rows32}
    assert sorted(r["name"] for r in rows16) == sorted(by32)
    for r in rows16:
        for k in ("mIoU", "mAcc", "aAcc"):
            assert r["metric.direct.%s" % k] == by32[r["name"]]["metric.direct.%s" % k]
            assert math.isfinite(r["metric.fp16.%s" % k])
    # a follow-up 'top' rule ranks the file
    best = ModelSpace.load(str(wd / "test_supernet" / "metrics_fp16.json")).apply_rule(
        dict(type="sample", operation="top", key="metric.direct.mIoU", value=1)).rows
    assert len(best) == 1
    assert best[0]["metric.direct.mIoU"] == max(r["metric.direct.mIoU"] for r in rows32)
