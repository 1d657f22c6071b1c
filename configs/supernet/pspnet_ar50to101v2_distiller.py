# BASELINE config 3 (PSP decode head + aux FCN on the dynamic R50..R101 supernet) trained against a
# FIXED teacher: the reference's DynamicDistiller segmentor
# (gaiaseg/models/segmentors/dynamic_distiller.py:152-413).  The student is the
# supernet, one sampled subnet per step as in ./pspnet_ar50to101v2.py; the teacher is the same model
# at full size, frozen, loaded from a local checkpoint:
#   python tools/train_supernet.py configs/supernet/pspnet_ar50to101v2_distiller.py \
#       --cfg-options model.teacher_ckpt=<supernet or extracted-subnet checkpoint>
# Besides the heads' label losses the student gets `distill_loss_seg` (soft-target cross entropy of
# the two logit maps at the image size) and `pairwise_loss_seg` (affinity of the last backbone feature
# on the window the reference's slice selects).  The teacher config carries no test_cfg of its own: it
# is built with the student's.  The checkpoints hold the student only and are read by
# tools/test_supernet.py, tools/finetune_supernet.py and tools/extract_subnet.py with the plain
# ./pspnet_ar50to101v2.py.  The same `model` in a finetune config (../supernet/fcn_ar50to101v2_finetune.py
# shows the other keys) gives every fast-finetuned subnet the fixed teacher.
_base_ = ['./pspnet_ar50to101v2.py']
_conv = dict(type='DynConv2d')
_teacher = dict(
    type='DynamicEncoderDecoder',
    backbone=dict(type='DynamicResNet', in_channels=3, stem_width=64, body_depth=[4, 6, 29, 4],
                  body_width=[80, 160, 320, 640], num_stages=4, out_indices=(0, 1, 2, 3),
                  conv_cfg=_conv, norm_cfg=dict(type='DynSyncBN', requires_grad=True, group_size=1),
                  style='pytorch'),
    decode_head=dict(type='DynamicPSPHead', conv_cfg=_conv, in_channels=2560, in_index=3,
                     channels=512, pool_scales=(1, 2, 3, 6), dropout_ratio=0.1, num_classes=19,
                     norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)))
model = dict(
    type='DynamicDistiller',
    teacher_segmentor=_teacher,
    teacher_ckpt=None,            # --cfg-options model.teacher_ckpt=<local file>
    has_distill_loss=True, distill_loss_temperature=1, distill_loss_weight=1,
    has_pairwise_loss=True, pairwise_loss_temperature=1, pairwise_loss_weight=1)
