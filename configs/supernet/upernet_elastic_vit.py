# UPerNet head over DynamicMultiLevelNeck on the elastic ViT supernet (maxima = ViT-B/16: 768 wide, 12
# heads, 3 groups of 4 layers, feed-forward ratio 40), 512x1024 crops (2049 tokens), bs 2 / GPU.
# Features: layers 2, 4, 8 and 12 (the second and the last layer of group 1, the last of groups 2 and 3),
# resized by the neck to strides 4 / 8 / 16 / 32.  Stochastic depth is not implemented (drop_path stays 0)
# and the supernet trains with the runner's SGD.  The backbone takes inputs of img_size only, so
# evaluation slides a window of that size.  (The first base file is read for its schedule, data and
# runtime settings only; this file replaces the model.)
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/elastic_vit.py']
crop_size = (512, 1024)
model = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='ElasticTransformer', embed_dim=768, num_heads=12, feedforward_channels=3072,
                  num_layers=[4, 4, 4], patch_size=16, img_size=crop_size, in_channels=3, attn_drop=0.0,
                  proj_drop=0.0, drop_rate=0.0, drop_path=0.0, out_indices=[[1], None, None],
                  out_stages=[0, 1, 2]),
    neck=dict(type='DynamicMultiLevelNeck', in_channels=[768, 768, 768, 768], out_channels=768,
              scales=[4, 2, 1, 0.5], conv_cfg=dict(type='DynConv2d')),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[768, 768, 768, 768], in_index=[0, 1, 2, 3], channels=512,
                     pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=768,
                        in_index=2, channels=256, num_convs=1, concat_input=False,
                        dropout_ratio=0.1, num_classes=19,
                        norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                        loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False,
                                         loss_weight=0.4)))
data = dict(samples_per_gpu=2, workers_per_gpu=2,
            train=dict(type='SyntheticSegDataset', size=crop_size, num_classes=19))
test_cfg = dict(mode='slide', crop_size=crop_size, stride=(512, 1024))
