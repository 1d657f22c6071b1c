# The elastic ViT supernet of ./upernet_elastic_vit_adamw.py (AdamW recipe) trained against the teacher the
# reference's DynamicDistiller was written for: a frozen BEiT-B/16 UPerNet
# (gaiaseg/models/backbones/beit.py), loaded from a local checkpoint in the public
# BEiT semantic-segmentation key layout:
#   python tools/train_supernet.py configs/supernet/upernet_elastic_vit_distiller_beit.py \
#       --cfg-options model.teacher_ckpt=<BEiT-B UPerNet checkpoint at this crop size>
# The teacher runs forward only, under no_grad, at img_size = crop_size (a 32 x 64 patch window, 2049
# tokens; its relative-position tables must have that window's 8004 rows -- tables of another size are
# refused, not interpolated).  Its four pyramid maps have the strides of the student's neck (4 / 8 / 16 / 32)
# and 768 channels, so `pairwise_loss_seg` compares the two stride-32 maps and `distill_loss_seg` the two
# logit maps.  Checkpoints hold the student only and are read with ./upernet_elastic_vit_adamw.py.
_base_ = ['./upernet_elastic_vit_adamw.py']
crop_size = (512, 1024)
_teacher = dict(
    type='EncoderDecoder',
    backbone=dict(type='BEiT', img_size=crop_size, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                  mlp_ratio=4, qkv_bias=True, use_abs_pos_emb=False, use_rel_pos_bias=True,
                  init_values=0.1, drop_path_rate=0.1, out_indices=[3, 5, 7, 11]),
    decode_head=dict(type='DynamicUPerHead', conv_cfg=dict(type='DynConv2d'),
                     in_channels=[768, 768, 768, 768], in_index=[0, 1, 2, 3], channels=768,
                     pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)))
model = dict(
    type='DynamicDistiller',
    teacher_segmentor=_teacher,
    teacher_ckpt=None,            # --cfg-options model.teacher_ckpt=<local file>
    has_distill_loss=True, distill_loss_temperature=1, distill_loss_weight=1,
    has_pairwise_loss=True, pairwise_loss_temperature=1, pairwise_loss_weight=1)
