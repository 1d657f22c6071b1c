# tools/test_supernet.py with multi-scale + flip test-time augmentation: the model-space rules of
# fcn_ar50to101v2_test_supernet.py, evaluated on Cityscapes val the way segmentation numbers are
# reported (mmseg's MultiScaleFlipAug: six ratios of 2048x1024, each plain and mirrored -> 12 views per
# image, probabilities averaged).  Every view of an image is written by one
# gs_tta_views launch.  evaluation.num_batches is left unset: one pass over the val set per subnet.
# apply_input_shape does not combine with a ladder of views and is refused.
_base_ = ['./fcn_ar50to101v2_test_supernet.py']
data_root = 'data/cityscapes/'
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
tta_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(2048, 1024),
         img_ratios=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75], flip=True,
         transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                     dict(type='Normalize', **img_norm_cfg),
                     dict(type='ImageToTensor', keys=['img']),
                     dict(type='Collect', keys=['img'])]),
]
data = dict(
    samples_per_gpu=1,
    val=dict(type='CityscapesDataset19', data_root=data_root, img_dir='leftImg8bit/val',
             ann_dir='gtFine/val', pipeline=tta_pipeline),
    test=dict(type='CityscapesDataset19', data_root=data_root, img_dir='leftImg8bit/val',
              ann_dir='gtFine/val', pipeline=tta_pipeline))
evaluation = dict(_delete_=True, interval=8000, metric='mIoU')
