# LOFT R50-FPN with multi-scale training: the headline config with Resize drawing a scale between 768 and 1280 (keep_ratio) in
# front of RandomFlip -- the standard multi-scale recipe; a building's apparent size is the ground resolution, so the scale draw
# stands for imagery at 0.75x to 1.25x BONAI's.  NOBODY HAS TRAINED WITH THIS CONFIG: the schedule is the headline's, unchanged.
# Deviations from the reference's Resize (README, "Resize and Pad"): ONE scale per batch, not per sample; gt_offsets are scaled
# with the image.  Pad(size_divisor=64): padded sides that are multiples of 32 but not of 64 are refused by the dataset.
# tools/train.py reads the Resize, RandomFlip, RandomRotate and Pad entries of data.train.pipeline; the other entries name what
# bonai_amd/dataset.py and data.to_device_batch do and are not interpreted.
_base_ = './loft_foa_r50_fpn_2x_bonai.py'
data_root = 'data/BONAI/'
train_cities = ('shanghai', 'beijing', 'jinan', 'haerbin', 'chengdu')
data = dict(
    train=dict(
        type='BONAI',
        ann_file=[f'{data_root}coco/bonai_{c}_trainval.json' for c in train_cities],
        img_prefix=[f'{data_root}trainval/images/'] * len(train_cities),
        bbox_type='building',
        mask_type='roof',
        pipeline=[
            dict(type='LoadImageFromFile'),
            dict(type='LoadAnnotations', with_bbox=True, with_mask=True, with_offset=True),
            dict(type='Resize', img_scale=[(768, 768), (1280, 1280)], multiscale_mode='range', keep_ratio=True),
            dict(type='RandomFlip', flip_ratio=0.5, direction=['horizontal', 'vertical']),
            dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
            dict(type='Pad', size_divisor=64),
            dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_offsets']),
        ]))
