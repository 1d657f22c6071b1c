"""Per-subnet BatchNorm re-calibration.

A supernet's BatchNorm running statistics are blended over every subnet sampled in training: each
subnet reads the leading slice of one buffer.  Before a subnet is scored, ``BNCalibrator`` replaces
the slices its inference forward reads by the cumulative average of K calibration batches' statistics
(PyTorch's ``momentum=None`` rule after a reset: the mean of the batch means, the mean of the unbiased
batch variances), and puts the blended values back afterwards bit for bit:

    SAVE (save bank) -> K x {forward with momentum 1, fold into the accumulator bank}
                     -> WRITE (accumulator, 1/K) -> evaluate -> WRITE (save bank, 1)

The forwards run without a tape, BatchNorm on batch statistics and everything else in eval mode, in
the precision ``fp16_enabled`` asks for.  With momentum 1 the kernels' ``(1-m)*r + m*b`` leaves exactly
the batch's statistics in the buffers (for finite r), so the momentum -- a by-value kernel argument
and part of the conv_bn plan key -- does not change from batch to batch.  The folds are one
table-driven launch over all visited layers each (``gs_bn_calib_fold``, csrc/norm.hip).
"""
import contextlib

import torch

from ..hip import lib as _lib
from ..hip.runtime import current_stream_ptr
from .input_shape import rescale_batch

RECALIBRATE_KEYS = ("num_batches", "samples_per_gpu", "seed")


def parse_recalibrate_cfg(calib_cfg, samples_per_gpu=None):
    """``cfg.caliberate_bn`` (sic) -> dict(num_batches, samples_per_gpu, seed) of its ``recalibrate``
    entry, or None when there is none.  ``samples_per_gpu``: ``data.samples_per_gpu``, the default of
    the entry's own key."""
    rc = (calib_cfg or {}).get("recalibrate")
    if rc is None:
        return None
    if calib_cfg.get("use_minibatch_stats", False):
        raise ValueError("caliberate_bn.recalibrate and caliberate_bn.use_minibatch_stats contradict "
                         "each other: the first re-estimates the running statistics, the second "
                         "drops them")
    rc = dict(rc)
    unknown = sorted(set(rc) - set(RECALIBRATE_KEYS))
    if unknown:
        raise KeyError("caliberate_bn.recalibrate: unknown key(s) %s (have %s)"
                       % (", ".join(unknown), ", ".join(RECALIBRATE_KEYS)))
    if "num_batches" not in rc:
        raise KeyError("caliberate_bn.recalibrate needs num_batches")

    def positive_int(key, value):
        if isinstance(value, bool) or not isinstance(value, int) or value <= 0:
            raise ValueError("caliberate_bn.recalibrate.%s must be a positive int, got %r" % (key, value))
        return value

    spg = rc.get("samples_per_gpu")
    if spg is None:
        spg = samples_per_gpu
    if spg is not None:
        positive_int("samples_per_gpu", spg)
    seed = rc.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError("caliberate_bn.recalibrate.seed must be an int, got %r" % (seed,))
    return dict(num_batches=positive_int("num_batches", rc["num_batches"]), samples_per_gpu=spg,
                seed=seed)


def build_calibration_batches(cfg, device="cuda", num_classes=19, loader_factory=None, calib_cfg=None):
    """The K calibration batches of ``cfg.caliberate_bn.recalibrate``, resident on ``device``; None
    without that key.  They come from ``data.train`` through the training loader and pipeline (with
    its augmentation: the statistics match what the network was trained on), built with the entry's
    seed as rank 0 of a world of 1 whatever the launch, so every rank holds the same batches and
    arrives at the same statistics without a collective.  ``loader_factory``: build_dataloader's
    stand-in (tests).  ``calib_cfg``: the ``caliberate_bn`` entry to read instead of ``cfg``'s own."""
    rc = parse_recalibrate_cfg(calib_cfg if calib_cfg is not None else cfg.get("caliberate_bn"),
                               cfg.data.get("samples_per_gpu"))
    if rc is None:
        return None
    if rc["samples_per_gpu"] is None:
        raise KeyError("caliberate_bn.recalibrate: no samples_per_gpu here or in data")
    if loader_factory is None:
        from ..apis.train import build_dataloader as loader_factory
    loader = loader_factory(cfg.data["train"], rc["samples_per_gpu"], seed=rc["seed"], device=device,
                            num_classes=num_classes,
                            workers_per_gpu=cfg.data.get("workers_per_gpu", 2), train=True,
                            device_cache_gb=cfg.data.get("device_cache_gb"), rank=0, world=1)
    it = iter(loader)
    batches = []
    for _ in range(rc["num_batches"]):
        b = next(it)
        # (a loader may hand its buffers out again: the calibrator owns copies)
        batches.append(dict(img=b["img"].detach().clone(), img_metas=list(b.get("img_metas") or ())))
    close = getattr(loader, "close", None)
    if close is not None:
        close()
    return batches


class _LayerTable:
    """The visited BatchNorm modules of one (arch, input size), their active widths, and the device
    table + banks the fold launches take."""
    __slots__ = ("mods", "widths", "ptrs", "table", "n", "floats", "save", "acc")


class BNCalibrator:
    """Re-calibrates the current subnet of ``model`` over ``batches`` (a list of dicts whose ``img``
    is a device tensor [N, 3, H, W]; ``img_metas`` is only read when a batch is rescaled).  The
    batches stay resident and are reused for every subnet: a subnet's calibrated statistics do not
    depend on which subnets were calibrated before it."""

    def __init__(self, model, batches):
        batches = list(batches)
        if not batches:
            raise ValueError("BNCalibrator needs at least one calibration batch")
        for b in batches:
            if not isinstance(b, dict) or not torch.is_tensor(b.get("img")):
                raise TypeError("a calibration batch is a dict with an 'img' tensor")
        self.model = model
        self.batches = batches
        self._tables = {}

    # ---- the subnet's inference forward: backbone + decode_head, no auxiliary head, no epilogue ----
    def _forward(self, img):
        model = self.model
        with torch.no_grad(), model._test_precision():
            return model._decode_head_forward_test(model.extract_feat(img), None)

    def _batch(self, k, input_shape):
        b = self.batches[k]
        if input_shape is None:
            return b["img"]
        n = int(b["img"].shape[0])
        full = dict(img=b["img"], img_metas=b.get("img_metas") or [dict() for _ in range(n)])
        return rescale_batch(full, input_shape, with_labels=False)[0]["img"]

    def _arch_key(self):
        bk = getattr(self.model, "backbone", None)
        state = bk.state_dict_of_arch() if hasattr(bk, "state_dict_of_arch") else None
        return repr(sorted(state.items())) if isinstance(state, dict) else repr(state)

    def _discover(self, img):
        """One eval-mode forward that records every ``bn_params(c)`` call: which BatchNorm layers the
        subnet visits and at which width, before any running statistic is written."""
        from .bricks import DynamicBatchNorm2d
        seen = {}
        patched = []
        for m in self.model.modules():
            if isinstance(m, DynamicBatchNorm2d) and m.running_mean is not None:
                def recorder(c, _m=m, _orig=m.bn_params):
                    seen[_m] = max(int(c), seen.get(_m, 0))
                    return _orig(c)
                m.__dict__["bn_params"] = recorder
                patched.append(m)
        try:
            self._forward(img)
        finally:
            for m in patched:
                m.__dict__.pop("bn_params", None)
        return list(seen.items())

    def _table(self, img):
        key = (self._arch_key(), tuple(img.shape))
        t = self._tables.get(key)
        if t is not None and t.ptrs == tuple(
                p for m in t.mods for p in (m.running_mean.data_ptr(), m.running_var.data_ptr())):
            return t
        layers = self._discover(img)
        if not layers:
            raise RuntimeError("BatchNorm re-calibration: the subnet's forward visits no BatchNorm "
                               "layer with running statistics")
        t = _LayerTable()
        t.mods = [m for m, _ in layers]
        t.widths = [c for _, c in layers]
        t.n = len(layers)
        host = (_lib.BnCalibLayer * t.n)()
        off, ptrs = 0, []
        for e, (m, c) in zip(host, layers):
            e.running_mean, e.running_var = m.running_mean.data_ptr(), m.running_var.data_ptr()
            e.channels, e.offset = c, off
            ptrs += [e.running_mean, e.running_var]
            off += 2 * c
        t.ptrs, t.floats = tuple(ptrs), off
        dev = img.device
        raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8)
        t.table = raw.to(dev)
        t.save = torch.empty(off, dtype=torch.float32, device=dev)
        t.acc = torch.empty(off, dtype=torch.float32, device=dev)
        if len(self._tables) > 256:
            self._tables.clear()
        self._tables[key] = t
        return t

    @staticmethod
    def _fold(t, bank, op, scale=1.0):
        _lib.check(_lib.load().gs_bn_calib_fold(t.table.data_ptr(), t.n, bank.data_ptr(), t.floats, op,
                                                scale, current_stream_ptr()), "gs_bn_calib_fold")

    def _calibrate(self, t, input_shape):
        """K forwards on batch statistics with momentum 1, each folded into the accumulator bank, then
        the average into the running buffers.  The modules' flags, momentum, statistics scope and
        host-side batch counters are as found afterwards, whatever happens."""
        found = [(m, m.training, m.momentum, m.sync, m.__dict__.get("_nbt_pending")) for m in t.mods]
        try:
            for m in t.mods:
                m.training, m.momentum, m.sync = True, 1.0, None   # rank-local batch statistics
                m.__dict__.pop("_bnp_cache", None)
            for k in range(len(self.batches)):
                self._forward(self._batch(k, input_shape))
                self._fold(t, t.acc, _lib.BN_CALIB_SAVE if k == 0 else _lib.BN_CALIB_ADD)
            self._fold(t, t.acc, _lib.BN_CALIB_WRITE, 1.0 / len(self.batches))
        finally:
            for m, training, momentum, sync, pending in found:
                m.training, m.momentum, m.sync = training, momentum, sync
                d = m.__dict__
                d.pop("_bnp_cache", None)
                if pending is None:
                    d.pop("_nbt_pending", None)
                else:
                    d["_nbt_pending"] = pending

    @contextlib.contextmanager
    def calibrated(self, input_shape=None):
        """Inside the block the model is in eval mode and the current subnet reads calibrated running
        statistics; after it the supernet is bit-identical to what it was before, parameters, buffers
        and module flags, also when the block (or the calibration itself) raises.  ``input_shape``: a
        ``data.input_shape`` value the calibration batches are resampled to (rescale_batch)."""
        model = self.model
        flags = [(m, m.training) for m in model.modules()]
        model.eval()
        saved = None
        try:
            t = self._table(self._batch(0, input_shape))
            self._fold(t, t.save, _lib.BN_CALIB_SAVE)
            saved = t
            self._calibrate(t, input_shape)
            yield self
        finally:
            if saved is not None:
                self._fold(saved, saved.save, _lib.BN_CALIB_WRITE, 1.0)
            for m, training in flags:
                m.training = training
