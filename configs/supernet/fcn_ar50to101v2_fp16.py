# BASELINE config 2 (FCN decode head + aux FCN on the dynamic R50..R101 supernet) trained with fp16
# conv operands, as mmseg's fp16 configs turn it on: mmcv's Fp16OptimizerHook with a static loss scale.
# The forward and data-gradient convolutions contract fp16-rounded operands with fp32 accumulation;
# activations, BatchNorm, loss, weight gradients and SGD stay fp32.
_base_ = ['./fcn_ar50to101v2.py']
optimizer_config = dict(type='Fp16OptimizerHook', loss_scale=512.)
# mmseg's placeholder: on its own it only means fp16 evaluation (tools/test_supernet.py)
fp16 = dict()
