# UPerNet head on the dynamic ConvNeXt V2 Nano..Base supernet (maxima = V2-Base), 512x1024 crops, bs 2 / GPU,
# trained with the AdamW recipe of upernet_convnext_t2b_adamw.py: decoupled weight decay 0.05 on the fused
# arena kernel, no decay on LayerNorm / BatchNorm parameters, a 1500-iteration linear warm-up into a linear
# ("poly", power 1) schedule.  The GRN weight and bias are not decayed either, as upstream.  Stochastic
# depth and layer-wise learning-rate decay are not implemented.  (The first base file is read for its
# schedule, data and runtime settings only; this file replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/convnextv2_n2b.py']
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicConvNeXtV2', depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024],
                  drop_path_rate=0.0, out_indices=[0, 1, 2, 3]),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], channels=512,
                     pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=512,
                        in_index=2, channels=256, num_convs=1, concat_input=False,
                        dropout_ratio=0.1, num_classes=19,
                        norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                        loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                         loss_weight=0.4)))
crop_size = (512, 1024)
data = dict(samples_per_gpu=2, workers_per_gpu=2,
            train=dict(type='SyntheticSegDataset', size=crop_size, num_classes=19))
optimizer = dict(_delete_=True, type='AdamW', lr=1e-4, betas=(0.9, 0.999), weight_decay=0.05,
                 paramwise_cfg=dict(norm_decay_mult=0., custom_keys={'grn': dict(decay_mult=0.)}))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
