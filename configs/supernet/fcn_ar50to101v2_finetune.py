# Fast-finetune with tools/finetune_supernet.py on the FCN supernet (configs/supernet/fcn_ar50to101v2.py):
# the third step of the workflow.  The model space is the file tools/test_supernet.py wrote (the rows
# of tools/count_flops.py plus metric.direct.*); the rule keeps the best rows of that pre-filter, every
# one of them is trained for runner.max_iters iterations from the supernet's weights as a one-anchor
# run and evaluated again, and the rows come back with metric.finetune.* next to metric.direct.*
# (gaia_seg_amd/apis/finetune.py).  The winner is then
#   dict(type='sample', operation='top', key='metric.finetune.mIoU', value=1)
# and tools/extract_subnet.py cuts it out (of the supernet, or of a --keep-checkpoints file).
# optimizer.lr=0 turns the run into a BatchNorm re-calibration of every subnet (no weight moves).
_base_ = ['./fcn_ar50to101v2.py']
model_space_path = None   # or --model-space-path: <work-dir>/test_supernet/metrics.json
model_sampling_rules = dict(type='sample', operation='top', key='metric.direct.mIoU', value=8,
                            mode='number')
load_from = None          # or --load-from: the supernet checkpoint
optimizer = dict(type='SGD', lr=0.001, momentum=0.9, weight_decay=0.0005)
lr_config = dict(policy='poly', power=0.9, min_lr=1e-5, by_epoch=False)
runner = dict(type='IterBasedRunner', max_iters=500)
log_config = dict(interval=50, hooks=[dict(type='TextLoggerHook', by_epoch=False)])
evaluation = dict(interval=500, metric='mIoU', num_batches=4)
