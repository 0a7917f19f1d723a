# The from-scratch recipe (loft_foa_r50_fpn_scratch_2x_bonai.py: nothing frozen, no ImageNet checkpoint) under the fused AdamW
# instead of momentum SGD, with no weight decay on norm scales / shifts and on biases (mmcv's paramwise_cfg).
# NOBODY HAS TRAINED WITH THESE NUMBERS: lr=1e-4 / weight_decay=0.05 are the customary AdamW starting point for detectors, not a
# tuned result of this project -- expect to search the learning rate.  The schedule (warm-up, steps at epochs 16 and 22) is the
# base config's.
_base_ = './loft_foa_r50_fpn_scratch_2x_bonai.py'
optimizer = dict(
    _delete_=True,
    type='AdamW', lr=0.0001, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05,
    paramwise_cfg=dict(norm_decay_mult=0., bias_decay_mult=0.))
optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))
