# ./pspnet_ar50to101v2_distiller.py with the channel-wise distillation loss (Shu et al., ICCV 2021;
# mmrazor's ChannelWiseDivergence) in place of the pairwise loss: every class map
# of the student's and the teacher's low-resolution logits becomes a distribution over its pixels, and
# `channel_loss_seg` is their KL divergence.  Temperature 1 and weight 5 are mmrazor's segmentation
# setting.  The teacher must have the student's output stride (the logit loss alone accepts another).
#   python tools/train_supernet.py configs/supernet/pspnet_ar50to101v2_distiller_cwd.py \
#       --cfg-options model.teacher_ckpt=<supernet or extracted-subnet checkpoint>
# The same three keys in the `model` of a finetune config give every fast-finetuned subnet the loss.
_base_ = ['./pspnet_ar50to101v2_distiller.py']
model = dict(
    has_pairwise_loss=False,
    has_channel_loss=True, channel_loss_temperature=1, channel_loss_weight=5)
