# The elastic ViT supernet of upernet_elastic_vit.py trained the way ViT segmentors are trained: AdamW
# with decoupled weight decay (the fused arena kernel gs_adamw_step_groups), no
# decay on LayerNorm / BatchNorm parameters, pos_embed and cls_token, and a 1500-iteration linear
# warm-up into a linear ("poly", power 1) schedule.  Layer-wise lr decay is not applied (a ViT-B
# layer-wise grouping needs more than the 16 groups of the hyper table).
_base_ = ['./upernet_elastic_vit.py']
optimizer = dict(_delete_=True, type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01,
                 paramwise_cfg=dict(custom_keys={'pos_embed': dict(decay_mult=0.),
                                                 'cls_token': dict(decay_mult=0.)},
                                    norm_decay_mult=0.))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
