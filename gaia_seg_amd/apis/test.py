"""Test-time drivers — host-side mirror of gaiaseg/apis/test.py:30-186 and the BatchNorm
re-calibration switches of gaiaseg/apis/train.py:177-184 / tools/test_supernet.py:190-198.

What differs by design: label maps stay on the device until a rank's shard is complete, and the
per-rank result lists are exchanged as python objects over the gloo host group
(``core.dist.gather_objects``) instead of pickled bytes staged through padded CUDA tensors
(collect_results_gpu, :155-186) or a shared tmp dir (collect_results_cpu, :113-152); the ordering
contract is the reference's: rank r holds samples r, r + world, ... and rank 0 returns them
interleaved and truncated to the dataset size."""
import torch
from torch.nn.modules.batchnorm import _BatchNorm

from ..core import dist as gdist


def apply_bn_calibration(model, calib_cfg, phase):
    """``cfg.caliberate_bn`` (sic — the reference's key).

    phase 'train' — ``reset_stats``: running_mean <- 0, running_var <- 1 before the run
                    (gaiaseg/apis/train.py:177-184);
    phase 'test'  — ``use_minibatch_stats``: drop the running statistics so that eval-mode BN
                    normalises with the statistics of the batch it sees
                    (tools/test_supernet.py:190-198)."""
    if not calib_cfg:
        return 0
    n = 0
    for m in model.modules():
        if not isinstance(m, _BatchNorm):
            continue
        if phase == "train" and calib_cfg.get("reset_stats", False):
            with torch.no_grad():
                m.running_mean.zero_()
                m.running_var.fill_(1)
            n += 1
        elif phase == "test" and calib_cfg.get("use_minibatch_stats", False):
            m.running_mean = None
            m.running_var = None
            m.track_running_stats = False
            # DynamicBatchNorm2d caches one BNParams view per mode holding the OLD buffers (ops.conv_bn
            # decides "batch statistics?" from that view): an eval forward before the calibration
            # would otherwise keep normalising with the running statistics
            m.__dict__.pop("_bnp_cache", None)
            n += 1
    return n


def _batch_results(model, data, **kw):
    with torch.no_grad():
        return model(return_loss=False, **data, **kw)


def single_gpu_test(model, data_loader, **kw):
    """gaiaseg/apis/test.py:30-88 without the visualisation branch: list of label maps."""
    model.eval()
    results = []
    for data in data_loader:
        out = _batch_results(model, data, **kw)
        results.extend(out if isinstance(out, list) else [out])
    return results


def collect_results(result_part, size):
    """Rank 0 gets the results of all ranks in dataset order (sample i lives on rank i % world at
    position i // world, the DistributedSampler layout); other ranks get None."""
    if not gdist.is_dist():
        return list(result_part)[:size]
    parts = gdist.gather_objects(list(result_part))
    if gdist.rank() != 0:
        return None
    ordered = []
    longest = max(len(p) for p in parts)
    for i in range(longest):
        for p in parts:
            if i < len(p):
                ordered.append(p[i])
    return ordered[:size]      # the sampler may have padded the last round


def multi_gpu_test(model, data_loader, size=None, **kw):
    """gaiaseg/apis/test.py:91-130: every rank evaluates its shard, rank 0 returns all results."""
    part = single_gpu_test(model, data_loader, **kw)
    if size is None:
        size = len(part) * gdist.world_size()
    return collect_results(part, size)


def test_model_space(model, loader, metas, num_batches, num_classes, ignore_index=255,
                     calib_cfg=None, metric_tag="direct", logger=None, apply_input_shape=None,
                     calibrator=None):
    """Evaluate every subnet of a model space (the loop of the reference's tools/test_supernet.py).

    For each flat meta: ``manipulate_arch`` with its arch, ``apply_bn_calibration(.., 'test')`` with
    ``calib_cfg`` (``cfg.caliberate_bn``: use_minibatch_stats), then ``core.evaluation.evaluate_model``
    over ``num_batches`` batches of ``loader`` (on-device confusion matrix, one all-reduce when
    distributed: every rank returns the same rows).  Returns one row per meta: the meta (other
    metric tags included) plus ``metric.<tag>.mIoU`` / ``.mAcc`` / ``.aAcc``.  The model's
    ``fp16_enabled`` (core.fp16_utils.wrap_fp16_model) decides the conv precision.
    ``apply_input_shape``: a row that carries ``data.input_shape`` is evaluated at that size
    (DESIGN.md section 20); without it the column is carried, not applied.  None (the default, what
    tools/test_supernet.py passes) reads the top-level ``apply_input_shape`` of the config the model
    was built from (``model.top_cfg``, models/builder.py).
    ``calibrator`` (core.bn_calibration.BNCalibrator over this model): every row is evaluated inside
    ``calibrator.calibrated(...)``, i.e. with BatchNorm running statistics re-estimated for its subnet
    (at the row's ``data.input_shape`` when that is applied), and the supernet is put back bit for bit
    before the next row.  Calibration is independent of the validation views, so test-time-augmentation
    loaders need nothing special.  Without a calibrator, a ``calib_cfg`` that carries ``recalibrate``
    (what tools/test_supernet.py passes: ``cfg.caliberate_bn``) builds one from the config the model was
    built from (``model.top_cfg``: its ``data.train`` supplies the calibration batches)."""
    import contextlib
    from ..core.bn_calibration import BNCalibrator, build_calibration_batches, parse_recalibrate_cfg
    if calibrator is None and parse_recalibrate_cfg(calib_cfg) is not None:
        top = getattr(model, "top_cfg", None)
        if top is None or top.get("data") is None:
            raise ValueError("caliberate_bn.recalibrate needs the calibration batches: pass a "
                             "calibrator, or build the model from a config that has data.train")
        calibrator = BNCalibrator(model, build_calibration_batches(
            top, device=next(model.parameters()).device, num_classes=num_classes, calib_cfg=calib_cfg))
    from ..core.dynamic import fold_dict
    from ..core.evaluation import check_tta_input_shape, evaluate_model
    from ..core.input_shape import INPUT_SHAPE_KEY
    from ..core.model_space import _listify, parse_input_shape
    if apply_input_shape is None:
        apply_input_shape = bool((getattr(model, "top_cfg", None) or {}).get("apply_input_shape", False))
    check_tta_input_shape(loader, apply_input_shape)
    if apply_input_shape:      # a bad value is refused before the first subnet is evaluated
        for meta in metas:
            if meta.get(INPUT_SHAPE_KEY) is not None:
                parse_input_shape(meta[INPUT_SHAPE_KEY])
    apply_bn_calibration(model, calib_cfg, "test")
    rows = []
    for i, meta in enumerate(metas):
        model.manipulate_arch(_listify(fold_dict(meta).get("arch", {})))
        input_shape = meta.get(INPUT_SHAPE_KEY) if apply_input_shape else None
        with (calibrator.calibrated(input_shape) if calibrator is not None
              else contextlib.nullcontext()):
            res = evaluate_model(model, loader, num_batches, num_classes, ignore_index,
                                 input_shape=input_shape)
        row = dict(meta)
        for k in ("mIoU", "mAcc", "aAcc"):
            row["metric.%s.%s" % (metric_tag, k)] = res[k]
        rows.append(row)
        if logger is not None and gdist.rank() == 0:
            logger.info("subnet %d/%d %s: mIoU %.4f mAcc %.4f aAcc %.4f"
                        % (i + 1, len(metas), meta.get("name", i), res["mIoU"], res["mAcc"], res["aAcc"]))
    return rows
