# UPerNet head on the dynamic ConvNeXt-T..B supernet (maxima = ConvNeXt-B), 512x1024 crops, bs 2 / GPU.
# Stochastic depth is not implemented (drop_path_rate stays 0) and the supernet trains with the
# runner's SGD, not the AdamW of the ConvNeXt recipe.  (The first base file is read for its schedule,
# data and runtime settings only; this file replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/convnext_t2b.py']
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicConvNeXt', depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024],
                  drop_path_rate=0.0, out_indices=[0, 1, 2, 3], layer_scale_init_value=1e-6,
                  conv_cfg=dict(type='DynConv2d')),
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
