# Model-space ranking with tools/test_supernet.py on the FCN supernet (configs/supernet/fcn_ar50to101v2.py).
# The model space is a file written by tools/count_flops.py (one flat meta per subnet with
# overhead.flops, counted at 512x2048); the rules below pick the subnets to evaluate
# (gaia_seg_amd/core/model_space.py build_sample_rule):
#   1. an R50-sized FLOPs band (R50 counts 238.5 GFLOPs, R101 393.7),
#   2. two groups by stage-3 depth (shallow <= 15 blocks, deep > 15),
#   3. two random subnets per group (seeded: the same draw on every rank),
#   4. the groups merged in order, duplicates dropped.
# A second round can rank the written metrics.json with
#   dict(type='sample', operation='top', key='metric.direct.mIoU', value=1).
# fp16 = dict(loss_scale=512.) would evaluate with fp16 conv operands (wrap_fp16_model).
_base_ = ['./fcn_ar50to101v2.py']
model_space_path = None   # or --model-space-path
model_sampling_rules = dict(
    type='sequential',
    rules=[
        dict(func_str="lambda x: 2.0e11 <= x['overhead.flops'] <= 4.0e11"),
        dict(type='parallel', rules=[
            dict(func_str="lambda x: x['arch.backbone.body.depth'][2] <= 15"),
            dict(func_str="lambda x: x['arch.backbone.body.depth'][2] > 15"),
        ]),
        dict(type='sample', operation='random', value=2, mode='number', seed=0),
        dict(type='merge'),
    ])
evaluation = dict(interval=8000, metric='mIoU', num_batches=4)
