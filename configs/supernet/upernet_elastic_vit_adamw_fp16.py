# upernet_elastic_vit_adamw.py trained in fp16: mmcv's Fp16OptimizerHook with a static loss scale (fp16
# operands in the convolutions and linears) and, opted into by fp16.attention, the
# fp16-operand attention kernels, forward and backward (gs_attention_*_f16).
# Activations, the softmax state, LayerNorm, the loss, weight gradients and AdamW stay fp32.
_base_ = ['./upernet_elastic_vit_adamw.py']
optimizer_config = dict(type='Fp16OptimizerHook', loss_scale=512.)
# Without the hook above this key would mean fp16 evaluation only (tools/test_supernet.py).
fp16 = dict(attention=True)
