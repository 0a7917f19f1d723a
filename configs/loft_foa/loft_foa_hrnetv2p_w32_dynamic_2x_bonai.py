# Config 5 (HRNetV2p-W32, binary16) with the dynamic loss scaler instead of the static 512: bonai_amd.engine.Trainer skips a step whose
# gradients overflowed, halves the scale, and doubles it again after 2000 clean steps (bonai_amd/loss_scale.py).  An extension: the
# reference's Fp16OptimizerHook knows only a static scale.
_base_ = './loft_foa_hrnetv2p_w32_2x_bonai.py'
fp16 = dict(loss_scale='dynamic')
