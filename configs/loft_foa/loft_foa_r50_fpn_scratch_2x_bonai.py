# LOFT R50-FPN trained from scratch: no ImageNet checkpoint and nothing frozen (frozen_stages=-1, mmdet's own default) -- the
# stem (conv1, bn1's gamma / beta) and layer1 learn with the rest.  For runs without a local checkpoint, where the headline
# config's frozen_stages=1 would freeze RANDOM features, and for fine-tuning on imagery with other band statistics.
_base_ = './loft_foa_r50_fpn_2x_bonai.py'
model = dict(
    pretrained=None,
    backbone=dict(frozen_stages=-1))
