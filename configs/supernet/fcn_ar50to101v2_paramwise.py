# BASELINE config 2 (FCN decode head + aux FCN on the dynamic R50..R101 supernet) with mmcv-style
# parameter groups: the two heads train at ten times the backbone's learning rate and BatchNorm
# parameters take no weight decay; linear warm-up over the first 500 iterations.  Every group follows
# the poly schedule from its own initial lr; the groups cut the arena into
# 77-269 fragments per anchor (MIN 77, R50 107, MAX 269), which one gs_sgd_step_groups launch per
# optimizer instalment covers.
_base_ = ['./fcn_ar50to101v2.py']
optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005,
                 paramwise_cfg=dict(custom_keys={'head': dict(lr_mult=10.)}, norm_decay_mult=0.))
lr_config = dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False,
                 warmup='linear', warmup_iters=500, warmup_ratio=1e-3)
