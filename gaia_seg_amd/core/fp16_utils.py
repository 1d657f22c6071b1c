"""fp16 inference switch, named after mmcv.runner.wrap_fp16_model (what the reference's
tools/test_supernet.py calls when the config has ``fp16 = dict(...)``).

mmcv casts the model to half and keeps fp16 activations between layers.  Here only the convolution
operands are rounded to fp16 (gs_set_forward_precision(1): fp16 MFMA, fp32 accumulation); the
activations stay fp32 in HBM, and BatchNorm, pooling, resize and the inference epilogue stay fp32.
This deviation is deliberate and strictly more accurate than the reference.
Training never reads it: ops.conv2d / ops.conv_bn refuse a recording tape in fp16 mode."""


def wrap_fp16_model(model):
    """Set ``fp16_enabled`` on every module that has the attribute (the segmentor: its simple_test,
    simple_test_device and aug_test then run inside ops.forward_precision('fp16')).  Returns the
    model.  A wrapper (DistributedDataParallel) is looked through by ``modules()``."""
    n = 0
    for m in model.modules():
        if hasattr(m, "fp16_enabled"):
            m.fp16_enabled = True
            n += 1
    if n == 0:
        raise ValueError("wrap_fp16_model: no module of %s has an fp16_enabled attribute"
                         % type(model).__name__)
    return model
