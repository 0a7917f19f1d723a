"""CPU: the contract of the fused mask -> RLE encoder (bonai_amd/csrc/mask_rle.hip) restated in numpy on the inputs the GPU tests use
(tests/mask_rle_restatement.py), the argument checks of tools/test.py and LoftRoIHead around it, and no CPU fallback."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_rle_restatement as M  # noqa: E402

from bonai_amd import rle as RL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 29


def _strings(h, w, S, thr, names=None, offsets=None, big=False):
    out = {}
    tnames, boxes, logits = M.big_table(S, h) if big else M.table(h, w, S)
    for i, name in enumerate(tnames):
        if names is not None and name not in names:
            continue
        mask = M.paste_np(M.sigmoid_np(logits[i]), boxes[i], h, w, thr)
        if offsets is not None:
            mask = M.translate_np(mask, offsets[i % len(offsets)])
        counts = M.counts_np(mask)
        s = RL.counts_to_string(counts)
        out[name] = (mask, counts, s)
    return out


@pytest.mark.parametrize('S', [28, 14])
@pytest.mark.parametrize('thr', [0.5, 0.3])
def test_restated_contract_round_trips_and_holds_every_kind(S, thr):
    got = _strings(H, W, S, thr)
    seen = set()
    for name, (mask, counts, s) in got.items():
        assert sum(counts) == H * W and all(c > 0 for c in counts[1:]), name
        assert RL.string_to_counts(s) == counts, name
        assert np.array_equal(RL.rle_decode({'size': [H, W], 'counts': s}), mask), name
        seen |= M.kinds(s, mask)
    assert got['cover_hi'][1] == [0, H * W]                      # one run through every column boundary
    assert got['interior_lo'][1] == [H * W]                      # the empty mask
    assert got['topleft_hi'][1][0] == 0                          # m[0] = 1
    assert got['bottomright_hi'][0][-1, -1] and got['stripe_hi'][0][[0, -1]].any(1).all()
    for name in ('zero_width', 'zero_height', 'zero_both', 'left_smooth', 'right_smooth', 'top_hi', 'bottom_hi', 'interior_smooth'):
        assert got[name][0].any(), name                          # the edge rows are no empty masks
    assert len(got['interior_alt'][1]) > 40                      # many short runs
    # a count of four characters needs 2^14 pixels: the 37 x 29 tile cannot hold one, the 1024^2 case below does
    assert seen == M.ALL_KINDS - {'four_chars'}, seen


def test_the_1024_case_holds_a_four_character_count():
    got = _strings(1024, 1024, 28, 0.5, big=True)
    seen = set()
    for name, (mask, counts, s) in got.items():
        assert RL.string_to_counts(s) == counts, name
        seen |= M.kinds(s, mask)
    assert len(got) == 4 and 4.5e5 < got['interior_smooth'][1][0] < 6e5 and seen == M.ALL_KINDS, seen


def test_restated_footprints():
    offs = np.array([[0, 0], [3.4, -2.6], [2.5, -2.5], [-7, 5], [W * .5, 3], [W + 3, -H]], np.float32)
    assert [M.round_half_away(v) for v in (2.5, -2.5, 3.4, -2.6, 0.49999, -0.5)] == [3, -3, 3, -3, 0, -1]
    roofs = _strings(H, W, 28, 0.5, names=('interior_smooth',))['interior_smooth'][0]
    ys, xs = np.nonzero(roofs)
    for off in offs:
        ox, oy = M.round_half_away(off[0]), M.round_half_away(off[1])
        foot = M.translate_np(roofs, off)
        want = np.zeros_like(roofs)
        keep = (ys - oy >= 0) & (ys - oy < H) & (xs - ox >= 0) & (xs - ox < W)       # footprint(y, x) = roof(y + oy, x + ox)
        want[ys[keep] - oy, xs[keep] - ox] = True
        assert np.array_equal(foot, want)
        s = RL.counts_to_string(M.counts_np(foot))
        assert np.array_equal(RL.rle_decode({'size': [H, W], 'counts': s}), foot)
    assert 0 < M.translate_np(roofs, offs[4]).sum() < roofs.sum()                   # partly out
    assert M.counts_np(M.translate_np(roofs, offs[5])) == [H * W]                   # wholly out


def _tools_test():
    spec = importlib.util.spec_from_file_location('loft_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('flags, word', [(['--fused-rle', '--eval'], '--eval'), (['--footprints', '--eval'], '--eval'),
                                         (['--fused-rle', '--bitmap-masks'], '--bitmap-masks'),
                                         (['--footprints', '--bitmap-masks'], '--bitmap-masks')])
def test_tools_test_py_refuses_combinations_before_building_a_model(flags, word, monkeypatch, capsys):
    import bonai_amd.loft as loft
    T = _tools_test()
    monkeypatch.setattr(loft, 'build_detector', lambda *a, **k: pytest.fail('a model was built'))
    monkeypatch.setattr(sys, 'argv', ['test.py', os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'),
                                      '--synthetic'] + flags)
    with pytest.raises(SystemExit) as e:
        T.main()
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert '--fused-rle' in err and word in err


def test_roi_head_refuses_inconsistent_result_modes():
    from bonai_amd.loft.roi import LoftRoIHead, _result_mode
    assert _result_mode({}) == (False, False) and _result_mode({'rle_masks': True}) == (False, False)
    assert _result_mode({'rle_masks': 'fused'}) == (True, False)
    assert _result_mode({'rle_masks': 'fused', 'footprint_rle': True}) == (True, True)
    bad = [({'rle_masks': 'fused', 'keep_device_masks': True}, 'keep_device_masks'), ({'footprint_rle': True}, "rle_masks='fused'"),
           ({'footprint_rle': True, 'rle_masks': True}, "rle_masks='fused'")]
    for cfg, word in bad:
        head = types.SimpleNamespace(test_cfg=cfg)
        with pytest.raises(ValueError, match=word):                      # before anything is computed
            LoftRoIHead.simple_test(head, None, None, None)
        with pytest.raises(ValueError, match=word):
            LoftRoIHead.aug_test(head, None, None, None, [0, 2])


def test_mask_paste_rle_has_no_cpu_fallback():
    from bonai_amd import kernels as K, lib as L
    with pytest.raises(L.LoftHipError):
        K.mask_paste_rle(torch.zeros(2, 28, 28), torch.tensor([[1., 1., 9., 9.], [2., 2., 8., 8.]]), 37, 29)
    with pytest.raises(L.LoftHipError):
        K.mask_paste_rle(torch.zeros(0, 28, 28), torch.zeros(0, 4), 37, 29)
