# SegFormer (arXiv 2105.15203): the all-MLP DynamicSegformerHead on the Mix Transformer supernet
# DynamicMixVisionTransformer (maxima = MiT-B3: depths 3/4/18/3, heads 1/2/5/8 of width 64, Mix-FFN ratio 4;
# subnets down to a MiT-B1-like net), 512x1024 crops, bs 2 / GPU: 32768 / 8192 / 2048 / 512 queries against
# 512 keys in the four stages (gs_attention_kv_*).  Trained as SegFormer is: AdamW
# (the fused arena kernel gs_adamw_step_groups), a 1500-iteration linear warm-up into a linear ("poly",
# power 1) schedule, no decay on norms, the heads at 10x the learning rate.  Stochastic depth is not
# implemented (drop_path_rate stays 0).  Nothing depends on an image size, so evaluation takes the whole
# image.  (The first base file is read for its schedule, data and runtime settings only; this file replaces
# the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/mit_b1to3.py']
crop_size = (512, 1024)
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicMixVisionTransformer', in_channels=3, num_stages=4, num_layers=[3, 4, 18, 3],
                  num_heads=[1, 2, 5, 8], patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2],
                  sr_ratios=[8, 4, 2, 1], mlp_ratio=4, out_indices=(0, 1, 2, 3), drop_rate=0.0,
                  attn_drop_rate=0.0, drop_path_rate=0.0),
    decode_head=dict(type='DynamicSegformerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[64, 128, 320, 512], in_index=[0, 1, 2, 3], channels=256,
                     dropout_ratio=0.1, num_classes=19, norm_cfg=dict(type='SyncBN', requires_grad=True),
                     align_corners=False,
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
