# The ConvNeXt supernet of upernet_convnext_t2b.py trained with AdamW (decoupled weight decay 0.05, the
# fused arena kernel gs_adamw_step_groups): no decay on LayerNorm / BatchNorm
# parameters, a 1500-iteration linear warm-up into a linear ("poly", power 1) schedule.  The upstream
# ConvNeXt recipe also decays the learning rate layer by layer (LearningRateDecayOptimizerConstructor);
# layer-wise decay is NOT applied here: every parameter trains at the one scheduled learning rate.
_base_ = ['./upernet_convnext_t2b.py']
optimizer = dict(_delete_=True, type='AdamW', lr=1e-4, betas=(0.9, 0.999), weight_decay=0.05,
                 paramwise_cfg=dict(norm_decay_mult=0.))
lr_config = dict(_delete_=True, policy='poly', power=1.0, min_lr=0.0, by_epoch=False,
                 warmup='linear', warmup_iters=1500, warmup_ratio=1e-6)
