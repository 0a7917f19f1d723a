"""GPU: validation while training (bonai_amd/validate.py, tools/train.py) on 256^2 tiles and a three-image annotation file.
The pass sees the weights the optimizer has just written, leaves the training run as it was, pastes only what the metric keeps
when asked to, and the tool writes the epoch / best checkpoints and the validation log."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py')
SIZE = 256
LOOSE = dict(score_thr=0.05, min_area=0)        # the synthetic weights' detections score low: let them into the records


def _cfg():
    from bonai_amd.config import Config
    return Config.fromfile(CFG)


def _synth_model():
    from bonai_amd.loft import build_detector
    from oracle.synth_weights import synth_tensor
    cfg = _cfg()
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    return m.cuda().train()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """Three 256^2 tiles with six well-separated axis-aligned buildings each (the construction of
    test_inference_gpu.py::test_dataset_evaluation_on_annotation_files, scaled down) -> (annotation file, tile directory)."""
    from PIL import Image
    d = tmp_path_factory.mktemp('val_tiles')
    rng = np.random.RandomState(0)
    images, annotations, aid = [], [], 0
    for i in range(3):
        name = f'tile_{i}.png'
        Image.fromarray(rng.randint(0, 255, (SIZE, SIZE, 3)).astype(np.uint8)).save(d / name, compress_level=1)
        images.append(dict(id=10 + i, file_name=name, width=SIZE, height=SIZE))
        k = 0
        while k < 6:
            w, h = rng.uniform(24, 60, 2)
            x, y = rng.uniform(15, SIZE - 80, 2)
            ox, oy = rng.uniform(-10, 10, 2)
            box = [x, y, x + w, y + h]
            if any(not (box[2] + 8 < b[0] or b[2] + 8 < box[0] or box[3] + 8 < b[1] or b[3] + 8 < box[1])
                   for b in (a['_box'] for a in annotations if a['image_id'] == 10 + i)):
                continue
            aid += 1
            k += 1
            annotations.append(dict(id=aid, image_id=10 + i, category_id=1, iscrowd=0, area=float(w * h), _box=box,
                                    bbox=[float(x), float(y), float(w), float(h)], roof_bbox=[float(x), float(y), float(w), float(h)],
                                    building_bbox=[float(x - 10), float(y - 10), float(w + 20), float(h + 20)],
                                    footprint_bbox=[float(x - ox), float(y - oy), float(w), float(h)],
                                    segmentation=[[float(v) for v in (x, y, x + w, y, x + w, y + h, x, y + h)]],
                                    footprint_mask=[float(v) for v in (x - ox, y - oy, x + w - ox, y - oy, x + w - ox, y + h - oy, x - ox, y + h - oy)],
                                    offset=[float(ox), float(oy)], building_height=10.0))
    f = d / 'bonai_val.json'
    json.dump(dict(images=images, annotations=annotations, categories=[dict(id=1, name='building')]), open(f, 'w'))
    return str(f), str(d)


@pytest.fixture(scope='module')
def ds(files):
    from bonai_amd.dataset import BonaiDataset
    return BonaiDataset(files[0], files[1], test_mode=True)


def _same_pass(a, b):
    """Two passes' (results, records): boxes, offsets and pairings identical, element for element."""
    (res_a, rec_a), (res_b, rec_b) = a, b
    assert len(res_a) == len(res_b) == len(rec_a) == len(rec_b) == 3
    for (bb_a, _, off_a), (bb_b, _, off_b) in zip(res_a, res_b):
        assert all(np.array_equal(x, y) for x, y in zip(bb_a, bb_b))
        assert np.array_equal(np.asarray(off_a, np.float32), np.asarray(off_b, np.float32))
    for ra, rb in zip(rec_a, rec_b):
        _same_record(ra, rb)


def _same_record(ra, rb):
    for name in ('roof', 'footprint'):
        for k in ('pred_TP', 'gt_TP', 'gt_FN', 'pred_FP'):
            assert ra[name][k] == rb[name][k], (name, k)
        assert np.array_equal(ra[name]['iou'], rb[name]['iou'])
    assert np.array_equal(ra['gt_offsets'], rb['gt_offsets']) and np.array_equal(ra['pred_offsets'], rb['pred_offsets'])
    assert ra['num_pred'] == rb['num_pred'] and ra['num_gt'] == rb['num_gt']


def test_validation_sees_the_current_weights(ds, tmp_path):
    """Two steps, a validation pass, a checkpoint: a FRESH model with that checkpoint loaded gives identical per-image results and
    records through the same loop -- and once more after two further steps.  The fused optimizer writes the arena through raw
    pointers (no Tensor._version moves): a pass that served folded / packed operands made before those writes fails here."""
    from bonai_amd.checkpoint import load_checkpoint, save_checkpoint
    from bonai_amd.engine import Trainer
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from bonai_amd.validate import Validator
    batches = [make_batch(2, SIZE, 8, step=s, device='cuda') for s in range(4)]
    m = _synth_model()
    tr = Trainer(m, lr=2e-2, momentum=0.9, weight_decay=1e-4, max_norm=35.0)
    v = Validator(m, ds, **LOOSE)
    passes = []
    for rnd in range(2):
        for s in (2 * rnd, 2 * rnd + 1):
            tr.train_step(batches[s])
        summary = v.run()
        assert m.training and set(summary) == {'roof', 'footprint', 'offset'}
        mine = (v.results, v.records)
        f = str(tmp_path / f'after_{rnd}.pth')
        save_checkpoint(m, f)
        cfg = _cfg()
        fresh = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        load_checkpoint(fresh, f, strict=True)
        vf = Validator(fresh.cuda().eval(), ds, **LOOSE)
        assert json.dumps(vf.run()) == json.dumps(summary)
        _same_pass(mine, (vf.results, vf.records))
        assert not fresh.training
        passes.append(mine)
        del fresh, vf
    n_det = [sum(b.shape[0] for b in r[0]) for r in passes[1][0]]
    print('detections per image in the second pass:', n_det)
    assert sum(n_det) > 0
    # the comparison has teeth: two further steps moved the detections
    assert any(not np.array_equal(a[0][0], b[0][0]) for a, b in zip(passes[0][0], passes[1][0]))


def _four_steps(batches, validate_after=None, ds=None):
    from bonai_amd import kernels as K
    from bonai_amd.engine import Trainer
    from bonai_amd.validate import Validator
    torch.manual_seed(0)
    K._SAMPLE_CALLS[0] = 0
    m = _synth_model()
    tr = Trainer(m, lr=2e-3, momentum=0.9, weight_decay=1e-4, max_norm=35.0, loss_scale='dynamic')
    logs = []
    for s in range(4):
        out = tr.train_step(batches[s], lr=2e-3 * (s + 1) / 4)
        logs.append({k: float(x) for k, x in out['log_vars'].items()})
        if validate_after is not None and s + 1 == validate_after:
            Validator(m, ds, **LOOSE).run()
            assert m.training
    torch.cuda.synchronize()
    idx = torch.randint(0, tr.arena.numel, (4096,), generator=torch.Generator().manual_seed(7)).cuda()
    ls = tr.loss_scale_state()
    return dict(logs=logs, params=tr.arena.data[idx].double().cpu().numpy(), calls=int(K._SAMPLE_CALLS[0]), iter=tr.iter, lr=tr.lr,
                scale={k: ls[k] for k in ('scale', 'good_steps', 'skipped', 'last_skipped')})


def test_training_is_undisturbed_by_a_validation_pass(ds):
    """Four steps with a validation pass after the second against four plain steps, same seeds: sampler draws, iteration counter,
    learning rate and loss-scale state equal; losses and a seeded sample of parameters within 4x the largest difference between
    TWO PLAIN four-step runs (what the atomics' summation order gives on unchanged code), floor one fp32 ulp of the value; if the
    two plain runs are bit-identical, bit-identical."""
    from bonai_amd.synth import make_batch
    batches = [make_batch(2, SIZE, 8, step=s, device='cuda') for s in range(4)]
    a = _four_steps(batches)
    b = _four_steps(batches)
    c = _four_steps(batches, validate_after=2, ds=ds)
    for k in ('calls', 'iter', 'lr', 'scale'):
        assert a[k] == b[k] == c[k], (k, a[k], b[k], c[k])
    assert a['calls'] > 0 and a['iter'] == 4
    keys = sorted(a['logs'][0])
    la, lb, lc = (np.asarray([[r[k] for k in keys] for r in x['logs']], np.float64) for x in (a, b, c))
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    for name, xa, xb, xc in (('losses', la, lb, lc), ('parameters', a['params'], b['params'], c['params'])):
        spread, got = float(np.abs(xa - xb).max()), np.abs(xa - xc)
        print(f'{name}: plain-vs-plain spread {spread:.3e}, with-validation-vs-plain max {float(got.max()):.3e}')
        if spread == 0.0:
            assert np.array_equal(xa, xc), name
        else:
            assert np.all(got <= np.maximum(4 * spread, ulp(xa))), (name, spread, float(got.max()))


def _image_pass(model, ds, eval_kw):
    """Every image through the model and evaluate_image -> [(3-tuple, pasted bitmaps, detections, record)]."""
    from bonai_amd import evaluation as E
    roi = model.roi_head
    out = []
    for i, data in ds.test_batches():
        with torch.no_grad():
            tup = model(return_loss=False, rescale=True, **data)
        n = sum(b.shape[0] for b in tup[0])
        pm = roi.last_device_masks if n else torch.zeros(0, SIZE, SIZE, dtype=torch.uint8, device='cuda')
        dets = roi.last_dets if n else np.zeros((0, 5), np.float32)
        offs = np.asarray(tup[2], np.float32).reshape(-1, 2) if n else np.zeros((0, 2), np.float32)
        out.append((tup, int(pm.shape[0]), np.array(dets), E.evaluate_image(pm, dets, offs, ds.get_ann_info(i), **eval_kw)))
    return out


def test_paste_min_score_keeps_what_the_metric_keeps(ds):
    """test_cfg.rcnn['paste_min_score']: the records of evaluate_image are those of the unset path, the number of pasted bitmaps is
    the number of detections at or above it, and with the key absent (again) simple_test returns the tuple it returned before."""
    m = _synth_model().eval()
    cfg = m.roi_head.test_cfg
    cfg['keep_device_masks'] = True
    cfg['rle_masks'] = True
    assert 'paste_min_score' not in cfg
    base = _image_pass(m, ds, dict(score_thr=0.4))
    scores = np.concatenate([d[:, 4] for _, _, d, _ in base])
    assert scores.size > 0
    median = float(np.median(scores))
    print(f'{scores.size} detections, scores {scores.min():.3f} .. {scores.max():.3f}, median {median:.3f}')
    for thr, kw in ((0.4, dict(score_thr=0.4)), (median, dict(score_thr=median, min_area=0))):
        want = _image_pass(m, ds, kw)
        cfg['paste_min_score'] = thr
        got = _image_pass(m, ds, kw)
        del cfg['paste_min_score']
        for (_, n_w, d_w, r_w), (tup, n_g, d_g, r_g) in zip(want, got):
            strong = d_w[:, 4] >= np.float32(thr)
            assert n_g == int(strong.sum()) == sum(b.shape[0] for b in tup[0]) and n_w == d_w.shape[0]
            assert np.array_equal(d_g, d_w[strong])
            _same_record(r_g, r_w)
        if thr == median:
            assert 0 < sum(g[1] for g in got) < sum(w[1] for w in want)         # (a real split: some pasted, some dropped)
    again = _image_pass(m, ds, dict(score_thr=0.4))
    for (t0, n0, _, _), (t1, n1, _, _) in zip(base, again):
        assert n0 == n1 and all(np.array_equal(x, y) for x, y in zip(t0[0], t1[0])) and t0[1] == t1[1]
        assert np.array_equal(np.asarray(t0[2], np.float32), np.asarray(t1[2], np.float32))


def _tool(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), CFG] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


def test_tools_train_py_validates_checkpoints_and_resumes(files, tmp_path):
    """tools/train.py on the tiny files: two epochs of two iterations with evaluation=dict(interval=1, save_best=...) -> the
    Epoch(val) lines, val.log.json, epoch_1 / epoch_2 / best / latest checkpoints; --resume-from epoch_1.pth continues at
    iteration 2; --no-validate writes no val.log.json."""
    ann, prefix = files
    work = tmp_path / 'work'
    common = ['--prefetch', '0', '--options', f'data.train.ann_file={ann}', f'data.train.img_prefix={prefix}',
              f'data.train.img_scale=({SIZE}, {SIZE})', 'data.samples_per_gpu=2', 'log_config.interval=1',
              'evaluation.save_best=footprint.F1_score', 'evaluation.score_thr=0.05', 'evaluation.min_area=0']
    val = ['--val-ann-file', ann, '--val-img-prefix', prefix]
    out = _tool(['--work-dir', str(work), '--iters', '4'] + val + common)
    for name in ('epoch_1.pth', 'epoch_2.pth', 'best.pth', 'latest.pth'):
        assert (work / name).exists(), (name, out[-1500:])
    lines = [json.loads(x) for x in open(work / 'val.log.json').read().splitlines()]
    assert len(lines) == 2 and [x['epoch'] for x in lines] == [1, 2] and [x['iter'] for x in lines] == [2, 4]
    for x in lines:
        assert {'roof', 'footprint', 'offset', 'best'} <= set(x) and {'F1_score', 'Precision', 'Recall', 'TP', 'FN', 'FP'} <= set(x['footprint'])
        assert {'aEPE', 'aAE', 'pairs'} <= set(x['offset']) and x['best']['key'] == 'footprint.F1_score'
        assert x['roof']['TP'] + x['roof']['FN'] >= 18
    vals = [x for x in out.splitlines() if x.startswith('Epoch(val)')]
    assert len(vals) == 2 and vals[0].startswith('Epoch(val) [1][3] roof_F1: ') and vals[1].startswith('Epoch(val) [2][3] ')
    assert 'pycocotools' in out                                          # the config's metric is the reference's ['bbox', 'segm']
    ck = torch.load(work / 'epoch_1.pth', map_location='cpu', weights_only=False)
    assert ck['meta']['iter'] == 2 and ck['meta']['epoch'] == 1 and ck['optimizer']['iter'] == 2 and ck['optimizer']['state']
    assert torch.load(work / 'latest.pth', map_location='cpu', weights_only=False)['meta']['iter'] == 4
    # resume: the next iteration is the first of epoch 2
    out = _tool(['--resume-from', str(work / 'epoch_1.pth'), '--iters', '3', '--no-validate'] + common)
    steps = [x for x in out.splitlines() if x.startswith('Epoch [')]
    assert len(steps) == 1 and steps[0].startswith('Epoch [2][1/2]'), out[-1500:]
    # --no-validate: checkpoints, no validation log, no Epoch(val) line
    work2 = tmp_path / 'work2'
    out = _tool(['--work-dir', str(work2), '--iters', '2', '--no-validate'] + val + common)
    assert (work2 / 'epoch_1.pth').exists() and (work2 / 'latest.pth').exists() and not (work2 / 'val.log.json').exists()
    assert 'Epoch(val)' not in out and not (work2 / 'best.pth').exists()
