#!/usr/bin/env python
"""Writes tests/golden/random_rotate.npz: inputs and outputs of the reference's own RandomRotate.bbox_rotate and
RandomRotate.offset_rotate (mmdet/datasets/pipelines/transforms.py:1957-2014) for the four right angles.

    BONAI_REFERENCE=/path/to/reference python tools/make_rotate_goldens.py

Runs on the CPU, where a checkout of the reference is at hand; the tests only read the fixture.  mmcv and cv2 are not
installed: oracle/ref_harness/mmcv_stub.py supplies the module stand-ins, and the one cv2 function bbox_rotate calls,
getRotationMatrix2D, is written here from OpenCV's documented formula.  imrotate is never called: for a right angle on a square
tile it is a pixel permutation (bonai_amd/data.py derives it), which is not what this fixture pins.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'ref_harness'))

ANGLES = (0, 90, 180, 270)
SIZE = 1024


def get_rotation_matrix_2d(center, angle, scale):
    """OpenCV's documented getRotationMatrix2D: alpha = scale * cos(angle), beta = scale * sin(angle), angle in degrees,
    [[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]] as float64."""
    rad = angle * math.pi / 180.0
    alpha, beta = scale * math.cos(rad), scale * math.sin(rad)
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def inputs():
    rng = np.random.RandomState(20)
    boxes = [[0, 0, 1024, 1024], [0, 0, 10, 20], [1000, 990, 1024, 1024], [0, 500, 37, 611], [400, 0, 512, 3],
             [512, 512, 512, 512], [17, 900, 17, 940], [300.5, 200.25, 340.75, 260.5], [511, 511, 513, 513]]
    for _ in range(15):
        x, y = rng.uniform(0, SIZE - 2, 2)
        boxes.append([x, y, rng.uniform(x + 1, SIZE), rng.uniform(y + 1, SIZE)])
    offsets = [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [37, 0], [0, -142], [-200, 0], [0, 200], [3, 4], [-5, 12], [141.5, -141.5],
               [0.25, -0.5], [-63, -16]]
    for _ in range(12):
        length, phi = rng.uniform(0.5, 200), rng.uniform(-math.pi, math.pi)
        offsets.append([length * math.cos(phi), length * math.sin(phi)])
    return np.array(boxes, dtype=np.float32), np.array(offsets, dtype=np.float32)


def main():
    import mmcv_stub
    mmcv_stub.install()
    sys.modules['cv2'].getRotationMatrix2D = get_rotation_matrix_2d
    from mmdet.datasets.pipelines.transforms import RandomRotate
    t = RandomRotate(rotate_ratio=1.0, choice=ANGLES)
    boxes, offsets = inputs()
    out = dict(angles=np.array(ANGLES, dtype=np.int64), img_shape=np.array([SIZE, SIZE, 3], dtype=np.int64), bboxes=boxes,
               offsets=offsets)
    for a in ANGLES:
        out[f'bboxes_{a}'] = np.asarray(t.bbox_rotate(boxes.copy(), (SIZE, SIZE, 3), a), dtype=np.float32)
        out[f'offsets_{a}'] = np.asarray(t.offset_rotate(offsets.copy(), (SIZE, SIZE, 3), a), dtype=np.float32)
        assert out[f'bboxes_{a}'].shape == boxes.shape and out[f'offsets_{a}'].shape == offsets.shape
    path = os.path.join(ROOT, 'tests', 'golden', 'random_rotate.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
