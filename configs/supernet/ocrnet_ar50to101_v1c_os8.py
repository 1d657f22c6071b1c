# OCRNet on the OS8 / "v1c" supernet of deeplabv3_ar50to101_v1c_os8.py: the same backbone and anchors
# with mmseg's ocrnet_r50-d8 cascade (CascadeEncoderDecoder: FCNHead on stage 3 -> OCRHead on stage 4,
# channels 512, ocr_channels 256) as DynamicFCNHead -> DynamicOCRHead.  Both stages have stride 8, so the
# FCN logits and the OCR features agree in size.  in_channels are the supernet maxima (4 x 320, 4 x 640);
# the active widths come with the feature maps.  No auxiliary head: stage 0 is the deep supervision.
_base_ = ['../_dynamic_/models/backbone_ar50to101v2.py', '../_dynamic_/model_samplers/ar50to101v2.py']
model = dict(
    type='DynamicCascadeEncoderDecoder',
    num_stages=2,
    backbone=dict(type='DynamicResNet', in_channels=3, stem_width=[32, 32, 64], deep_stem=True,
                  avg_down=False, body_depth=[4, 6, 29, 4], body_width=[80, 160, 320, 640],
                  num_stages=4, dilations=(1, 1, 2, 4), strides=(1, 2, 1, 1), contract_dilation=True,
                  out_indices=(0, 1, 2, 3), conv_cfg=dict(type='DynConv2d'),
                  norm_cfg=dict(type='DynSyncBN', requires_grad=True, group_size=1),
                  style='pytorch'),
    decode_head=[
        dict(type='DynamicFCNHead', conv_cfg=dict(type='DynConv2d'), in_channels=1280, in_index=2,
             channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1, num_classes=19,
             norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
             loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.4)),
        dict(type='DynamicOCRHead', conv_cfg=dict(type='DynConv2d'), in_channels=2560, in_index=3,
             channels=512, ocr_channels=256, dropout_ratio=0.1, num_classes=19,
             norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
             loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
    ])
train_cfg = dict()
test_cfg = dict(mode='whole')
# the deep stem takes a width per stem conv (reference anchors of psp_ar50to101_v1c_extract.py:78-113)
stem_anchors = dict(MAX=[32, 32, 64], MIN=[16, 16, 32], R50=[32, 32, 64], R77=[32, 32, 64],
                    R101=[32, 32, 64])
