"""CPU: the loop restatement of multiclass_nms with soft-NMS (tests/soft_select_restatement.py) -- the statement the GPU tests hold
kernels.multiclass_soft_nms_batched to -- against oracle.ops_ref.multiclass_nms bit for bit and against hand-derived cases; that the
shared batches reach what they are for; and SceneDetector's ``soft_nms_batched`` keyword."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_select_restatement as S  # noqa: E402
from test_det_select_cpu import _Stub  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize('method', ['naive', 'linear'])
@pytest.mark.parametrize('name,agnostic', S.variants())
def test_restatement_equals_the_oracle(name, agnostic, method):
    from oracle import ops_ref
    images, score_thr, iou_thr, k = S.batch(name)
    cfg = dict(type='soft_nms', iou_threshold=iou_thr, method=method, class_agnostic=agnostic)
    for (b, s), (wd, wl, _) in zip(images, S.want(name, method, agnostic)):
        if b.shape[0] == 0:                             # the per-image forms cannot view [0, 4C]
            assert wd.shape == (0, 5) and wl.shape == (0,)
            continue
        d, l = ops_ref.multiclass_nms(torch.from_numpy(b), torch.from_numpy(s), score_thr, cfg, k)
        assert np.array_equal(_bits(d.numpy()), _bits(wd)) and np.array_equal(l.numpy(), wl), name


@pytest.mark.parametrize('name', sorted(S.hand_cases()))
def test_hand_cases(name):
    bboxes, scores, score_thr, iou_thr, method, max_num, dets, labels = S.hand_cases()[name]
    d, l = S.multiclass_soft_nms(np.array(bboxes, np.float32), np.array(scores, np.float32), score_thr, iou_thr, method, max_num)
    assert np.array_equal(d, np.array(dets, np.float32).reshape(-1, 5)) and l.tolist() == labels


def test_the_inputs_reach_what_they_are_for():
    from bonai_amd import kernels as K
    hdr = open(os.path.join(ROOT, 'include', 'loft_hip.h')).read()
    assert K.SOFT_NMS_LDS_CAPACITY == S.CAPACITY == int(re.search(r'#define\s+LOFT_SOFT_NMS_LDS_CAPACITY\s+(\d+)', hdr).group(1))
    infos = {(n, m): [w[2] for w in S.want(n, m)] for n in S.NAMES for m in ('naive', 'linear')}
    # a drop step with holes and fillers (every filler fills a hole): under naive everywhere, under linear through the duplicates
    assert infos['three_c3_per_class', 'naive'][2]['fillers'] > 0
    assert infos['clustered_5000_duplicates', 'linear'][1]['fillers'] > 0 and infos['clustered_5000_duplicates', 'linear'][1]['drop_rounds'] > 0
    # the cut: below the number of selections, and above it
    k = S.batch('three_c3_per_class')[3]
    assert all(i[2]['selections'] > k for i in (infos['three_c3_per_class', 'naive'], infos['three_c3_per_class', 'linear']))
    k = S.batch('one_image_below_thr')[3]
    assert all(0 < i['selections'] < k for i in infos['one_image_below_thr', 'naive'][::2])
    assert infos['one_image_below_thr', 'linear'][1]['candidates'] == 0 < infos['one_image_below_thr', 'linear'][0]['candidates']
    k = S.batch('clustered_5000_duplicates')[3]
    assert infos['clustered_5000_duplicates', 'linear'][1]['selections'] > k            # the workspace form stops early
    # C = 3: flat order is not class-major order
    b, s = S.batch('three_c3_per_class')[0][2]
    flat = [f for _, f, _, _ in S.candidates(b, s, 0.05)]
    assert flat == sorted(flat) and flat != sorted(flat, key=lambda f: (f % 3, f // 3))
    # both forms of the state, and the capacity's two sides
    rows = {n: max(b.shape[0] for b, _ in S.batch(n)[0]) * S.classes(n) for n in S.NAMES}
    assert rows['capacity_rows'] == K.SOFT_NMS_LDS_CAPACITY and rows['capacity_plus_one_rows'] == K.SOFT_NMS_LDS_CAPACITY + 1
    assert rows['clustered_5000_duplicates'] > K.SOFT_NMS_LDS_CAPACITY
    assert infos['capacity_rows', 'linear'][0]['candidates'] > 3000 and infos['clustered_5000_duplicates', 'linear'][1]['candidates'] == 5000
    assert len(S.batch('sixteen_small')[0]) == 16
    sc = S.batch('ties_sixteenths')[0][1][1]
    assert np.array_equal(sc * 16, np.round(sc * 16)) and len(np.unique(sc)) <= 17


# ---------------------------------------------------------------------------------------------------------------- SceneDetector
def test_scene_detector_takes_soft_nms_in_batches_with_the_keyword():
    from bonai_amd.scene import SceneDetector
    det = SceneDetector(_Stub('soft_nms'), tile=64, overlap=32, batch=2, soft_nms_batched=True)
    assert det.batch == 2 and det.soft_nms_batched is True
    assert SceneDetector(_Stub('nms'), tile=64, overlap=32, batch=2, soft_nms_batched=True).batch == 2
    assert SceneDetector(_Stub('soft_nms'), tile=64, overlap=32, batch=1, soft_nms_batched=True).batch == 1
    assert SceneDetector(_Stub('soft_nms'), tile=64, overlap=32).soft_nms_batched is False


def test_scene_detector_refuses_as_before_without_the_keyword():
    from bonai_amd.scene import SceneDetector
    for kw in ({}, {'soft_nms_batched': False}):
        with pytest.raises(ValueError, match='batch=1'):
            SceneDetector(_Stub('soft_nms'), tile=64, overlap=32, batch=2, **kw)
    with pytest.raises(ValueError, match='batch=1'):                       # the keyword opts into soft-NMS, not into any other type
        SceneDetector(_Stub('other'), tile=64, overlap=32, batch=2, soft_nms_batched=True)


def test_scene_tool_refuses_both_flags(monkeypatch, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location('scene_tool', os.path.join(ROOT, 'tools', 'scene.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, 'argv', ['scene.py', 'cfg.py', 'img.png', '--out', 'o.pkl', '--batch', '2', '--hard-nms', '--batched-soft-nms'])
    with pytest.raises(SystemExit):
        tool.main()
    assert '--batched-soft-nms' in capsys.readouterr().err
