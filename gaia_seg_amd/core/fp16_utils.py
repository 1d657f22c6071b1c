"""fp16 switches, named after mmcv.runner's fp16_utils.

``wrap_fp16_model`` (what the reference's tools/test_supernet.py calls when the config has
``fp16 = dict(...)``, and what mmcv's Fp16OptimizerHook calls in before_run): fp16 inference.
mmcv casts the model to half and keeps fp16 activations between layers.  Here only the convolution
operands are rounded to fp16 (gs_set_forward_precision(1): fp16 MFMA, fp32 accumulation); the
activations stay fp32 in HBM, and BatchNorm, pooling, resize and the inference epilogue stay fp32.
This deviation is deliberate and strictly more accurate than the reference.
ops.conv2d / ops.conv_bn refuse a recording tape in that mode.

fp16 TRAINING is a separate switch (gs_set_train_precision, ops.train_precision) that the runner
sets around every step when ``optimizer_config = dict(type='Fp16OptimizerHook', loss_scale=...)``
(core/runner.py Fp16ArenaOptimizerHook).  ``LossScaler`` holds the loss scale
in mmcv's state_dict form, the form checkpoints carry under ``meta['fp16']['loss_scaler']``."""


def check_fp16_cfg(fp16):
    """A config's ``fp16`` value (None or a dict) -> whether it asks for fp16 attention:
    ``fp16 = dict(attention=True)``.  The key must be a bool."""
    attention = (fp16 or {}).get("attention", False)
    if not isinstance(attention, bool):
        raise ValueError("fp16.attention must be a bool, got %r" % (attention,))
    return attention


def wrap_fp16_model(model, attention=None):
    """Set ``fp16_enabled`` on every module that has the attribute (the segmentor: its simple_test,
    simple_test_device and aug_test then run inside ops.forward_precision('fp16')).  Returns the
    model.  A wrapper (DistributedDataParallel) is looked through by ``modules()``.

    ``attention=True`` also sets ``fp16_attention`` on every module that has it (ElasticTransformer, BEiT
    and their attention modules): inside an fp16 mode their attention then runs on the fp16-operand
    kernels.  A model without such a module raises ValueError: the switch would
    do nothing.  ``attention=None`` (the default, what tools/test_supernet.py's ``wrap_fp16_model(model)``
    gives) takes ``fp16 = dict(attention=...)`` of the config the model was built from
    (``model.top_cfg``, models/builder.py); a model built from a plain dict has no such config, and the
    switch stays off."""
    if attention is None:
        tops = [m.top_cfg for m in model.modules() if getattr(m, "top_cfg", None) is not None]
        attention = check_fp16_cfg(tops[0].get("fp16")) if tops else False
    n = 0
    for m in model.modules():
        if hasattr(m, "fp16_enabled"):
            m.fp16_enabled = True
            n += 1
    if n == 0:
        raise ValueError("wrap_fp16_model: no module of %s has an fp16_enabled attribute"
                         % type(model).__name__)
    if attention:
        mods = [m for m in model.modules() if hasattr(m, "fp16_attention")]
        if not mods:
            raise ValueError("wrap_fp16_model(attention=True): no module of %s has an fp16_attention "
                             "attribute (fp16 attention needs an ElasticTransformer or BEiT backbone)"
                             % type(model).__name__)
        for m in mods:
            m.fp16_attention = True
    return model


class LossScaler:
    """mmcv.runner.fp16_utils.LossScaler (mmcv-full 1.3.0, after apex): the scale, the iteration
    counters and the update rule, with mmcv's state_dict keys.  The training step uses a static
    scale (mode 'static': update_scale leaves it alone)."""

    def __init__(self, init_scale=2 ** 32, mode="dynamic", scale_factor=2., scale_window=1000):
        if mode not in ("dynamic", "static"):
            raise ValueError("mode can only be dynamic or static, got %r" % (mode,))
        self.cur_scale = init_scale
        self.cur_iter = 0
        self.mode = mode
        self.last_overflow_iter = -1
        self.scale_factor = scale_factor
        self.scale_window = scale_window

    @property
    def loss_scale(self):
        return self.cur_scale

    def update_scale(self, overflow):
        """After an overflowing step: scale / factor (at least 1); after scale_window clean steps
        since the last overflow: scale * factor.  Static mode: no change."""
        if self.mode == "static":
            return
        if overflow:
            self.cur_scale = max(self.cur_scale / self.scale_factor, 1)
            self.last_overflow_iter = self.cur_iter
        elif (self.cur_iter - self.last_overflow_iter) % self.scale_window == 0:
            self.cur_scale *= self.scale_factor
        self.cur_iter += 1

    def state_dict(self):
        return dict(cur_scale=self.cur_scale, cur_iter=self.cur_iter, mode=self.mode,
                    last_overflow_iter=self.last_overflow_iter, scale_factor=self.scale_factor,
                    scale_window=self.scale_window)

    def load_state_dict(self, state_dict):
        self.cur_scale = state_dict["cur_scale"]
        self.cur_iter = state_dict["cur_iter"]
        self.mode = state_dict["mode"]
        self.last_overflow_iter = state_dict["last_overflow_iter"]
        self.scale_factor = state_dict["scale_factor"]
        self.scale_window = state_dict["scale_window"]
