# UPerNet + Swin (arXiv 2103.14030): DynamicUPerHead on the Swin supernet DynamicSwinTransformer (maxima =
# Swin-B: depths 2/2/18/2, heads 4/8/16/32 of width 32, window 7, MLP ratio 4; subnets down to Swin-T), 512x1024
# crops, bs 2 / GPU: stage maps 128x256 .. 16x32, padded to the window inside every block
# (gs_window_attention_*).  Trained as Swin segmentors are: AdamW (the fused arena kernel
# gs_adamw_step_groups), a 1500-iteration linear warm-up into a linear ("poly", power 1) schedule, no decay on
# norms and on the relative-position tables, the heads at 10x the learning rate.  Stochastic depth is not
# implemented (drop_path_rate stays 0).  Nothing depends on an image size, so evaluation takes the whole image.
# (The first base file is read for its schedule, data and runtime settings only; this file replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/swin_t2b.py']
crop_size = (512, 1024)
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicSwinTransformer', in_channels=3, patch_size=4, window_size=7, mlp_ratio=4,
                  depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], out_indices=(0, 1, 2, 3), qkv_bias=True,
                  drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, use_abs_pos_embed=False,
                  norm_cfg=dict(type='LN', eps=1e-5)),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6),
                     channels=512, dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=512,
                        in_index=2, channels=256, num_convs=1, concat_input=False,
                        dropout_ratio=0.1, num_classes=19,
                        norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                        loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                         loss_weight=0.4)))
data = dict(samples_per_gpu=2, workers_per_gpu=2,
            train=dict(type='SyntheticSegDataset', size=crop_size, num_classes=19))
test_cfg = dict(mode='whole')
optimizer = dict(_delete_=True, type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01,
                 paramwise_cfg=dict(custom_keys={'head': dict(lr_mult=10.),
                                                 'relative_position_bias_table': dict(decay_mult=0.)},
                                    norm_decay_mult=0.))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
