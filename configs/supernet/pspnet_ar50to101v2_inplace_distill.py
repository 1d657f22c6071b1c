# BASELINE config 3 (PSP decode head + aux FCN on the dynamic R50..R101 supernet) trained with in-place
# distillation (tools/train_supernet.py:180-187): every iteration trains MAX, MIN and
# `sample_subnet_num` random subnets on the same batch -- MAX on the labels, the others against MAX's
# detached logits -- and takes one SGD step on the sum of their gradients (US-Nets' sandwich rule).
# The search space is the one of ../_dynamic_/model_samplers/ar50to101v2.py.
_base_ = ['./pspnet_ar50to101v2.py']
_stem = dict(key='arch.backbone.stem.width', start=32, end=64, step=16)
_width = dict(key='arch.backbone.body.width', start=[48, 96, 192, 384], end=[80, 160, 320, 640],
              step=[16, 32, 64, 128], ascending=True)
_depth = dict(key='arch.backbone.body.depth', start=[2, 2, 5, 2], end=[4, 6, 29, 4],
              step=[1, 2, 2, 1])
use_distillation = True
max_net = dict(type='anchor', anchors=[
    {'name': 'MAX', 'arch.backbone.stem.width': 64, 'arch.backbone.body.width': [80, 160, 320, 640],
     'arch.backbone.body.depth': [4, 6, 29, 4]}])
min_net = dict(type='anchor', anchors=[
    {'name': 'MIN', 'arch.backbone.stem.width': 32, 'arch.backbone.body.width': [48, 96, 192, 384],
     'arch.backbone.body.depth': [2, 2, 5, 2]}])
random_subnet = dict(type='composite', model_samplers=[dict(type='range', **_stem),
                                                       dict(type='range', **_width),
                                                       dict(type='range', **_depth)])
sample_subnet_num = 3
# the distillation branch's hyper-parameters, the reference's defaults
# (dynamic_psp_head.py:196-200, dynamic_fcn_head.py:181-185)
distill_cfg = dict(T=2.0, distillation_weight=0.5, interpolation=False)
