# UPerNet head on the SegNeXt supernet DynamicMSCAN (maxima = MSCAN-B: depths 3/3/12/3, widths 64/128/320/512,
# feed-forward ratios 8/8/4/4; subnets down to an MSCAN-T-like net), 512x1024 crops, bs 2 / GPU.  The seven
# depthwise filters of every block's spatial gating unit run as one operator (gs_msca_*, DESIGN.md section
# 40).  Trained with the AdamW recipe of segformer_mit_b1to3_adamw.py: the fused arena kernel, a
# 1500-iteration linear warm-up into a linear ("poly", power 1) schedule, no decay on norms, the heads at
# 10x the learning rate.  Nothing depends on an image size, so evaluation takes the whole image.
# Not implemented: SegNeXt's own decoder (LightHamHead, the NMF "hamburger"; the UPer head stands in),
# stochastic depth and dropout in the backbone (drop_path_rate and drop_rate stay 0), fp16 operands for the
# strip convolutions.  (The first base file is read for its schedule, data and runtime settings only; this
# file replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/mscan_t2b.py']
crop_size = (512, 1024)
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicMSCAN', in_channels=3, embed_dims=[64, 128, 320, 512], mlp_ratios=[8, 8, 4, 4],
                  depths=[3, 3, 12, 3], num_stages=4, drop_rate=0.0, drop_path_rate=0.0,
                  attention_kernel_sizes=[5, [1, 7], [1, 11], [1, 21]],
                  attention_kernel_paddings=[2, [0, 3], [0, 5], [0, 10]], act_cfg=dict(type='GELU'),
                  norm_cfg=dict(type='SyncBN', requires_grad=True), out_indices=(0, 1, 2, 3)),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[64, 128, 320, 512], in_index=[0, 1, 2, 3], channels=512,
                     pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=320,
                        in_index=2, channels=256, num_convs=1, concat_input=False,
                        dropout_ratio=0.1, num_classes=19,
                        norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                        loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                         loss_weight=0.4)))
data = dict(samples_per_gpu=2, workers_per_gpu=2,
            train=dict(type='SyntheticSegDataset', size=crop_size, num_classes=19))
test_cfg = dict(mode='whole')
optimizer = dict(_delete_=True, type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01,
                 paramwise_cfg=dict(custom_keys={'head': dict(lr_mult=10.)}, norm_decay_mult=0.))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
