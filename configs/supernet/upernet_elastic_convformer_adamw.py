# UPerNet head directly on the four maps (strides 4 / 8 / 16 / 32) of the elastic Conformer supernet
# (maxima = Conformer-B-like: embed 576, 9 heads, conv widths 384 / 768 / 1536, 3 + 4 + 4 + 1 blocks, ratio
# 4), no neck, FCN auxiliary head on stage 3, 512x1024 crops (2049 tokens), bs 2 / GPU.  Trained as the
# elastic ViT of upernet_elastic_vit_adamw.py: AdamW with decoupled weight decay (the fused arena kernel
# gs_adamw_step_groups), no decay on LayerNorm / BatchNorm parameters and cls_token,
# a 1500-iteration linear warm-up into a linear ("poly", power 1) schedule.  Stochastic depth is not
# implemented (drop_path stays 0).  norm_eval keeps the reference's value: the conv branch's BatchNorms use
# their running statistics (the supernet starts from a checkpoint; norm_eval=False trains them from
# scratch).  (The first base file is read for its schedule, data and runtime settings only; this file
# replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/elastic_convformer.py']
crop_size = (512, 1024)
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='ElasticConvformer', embed_dim=576, num_heads=[9, 9, 9], mlp_ratio=[4, 4, 4], depth=12,
                  stem_width=64, body_width=[384, 768, 1536], body_depth=[3, 4, 4], patch_size=16, in_chans=3,
                  proj_drop=0.0, attn_drop=0.0, drop_path=0.0, norm_eval=True),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[384, 768, 1536, 1536], in_index=[0, 1, 2, 3], channels=512,
                     pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=1536,
                        in_index=2, channels=256, num_convs=1, concat_input=False,
                        dropout_ratio=0.1, num_classes=19,
                        norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                        loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                         loss_weight=0.4)))
data = dict(samples_per_gpu=2, workers_per_gpu=2,
            train=dict(type='SyntheticSegDataset', size=crop_size, num_classes=19))
optimizer = dict(_delete_=True, type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01,
                 paramwise_cfg=dict(custom_keys={'cls_token': dict(decay_mult=0.)}, norm_decay_mult=0.))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
