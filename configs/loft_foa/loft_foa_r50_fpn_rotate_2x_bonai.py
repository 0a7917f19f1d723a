# LOFT R50-FPN with rotation augmentation: the headline config plus RandomRotate(rotate_ratio=0.5) after RandomFlip -- the
# image-level counterpart of the FOA head's four feature-level branches (same four angles).  A BONAI city has a single viewing
# angle, so every offset in it points the same way; flips give four of the square's eight symmetries, flips and right-angle
# rotations together all eight.  Right angles on the square 1024 tiles only ("RandomRotate").
# tools/train.py reads the two augmentation entries of data.train.pipeline, in their order; the other entries name what
# bonai_amd/dataset.py and data.to_device_batch do for the fixed-size tiles and are not interpreted.
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
            dict(type='RandomFlip', flip_ratio=0.5, direction=['horizontal', 'vertical']),
            dict(type='RandomRotate', rotate_ratio=0.5, choice=(0, 90, 180, 270)),
            dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
            dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels', 'gt_masks', 'gt_offsets']),
        ]))
