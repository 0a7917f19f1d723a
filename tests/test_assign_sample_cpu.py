"""CPU: the references, case tables and censuses of tests/assign_sample_restatement.py, which tests/test_assign_sample_gpu.py holds
loft_iou_assign and loft_random_sample to.  Nothing here runs a kernel: these tests establish that the references say what
oracle/ops_ref.py says, that the tables reach every path and edge they are meant to reach, that the committed tie seeds do tie, and
that the sampler's keys draw uniformly."""
import collections

import numpy as np
import torch

import assign_sample_restatement as R
from oracle import ops_ref


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
def _census():
    return {name: R.sample_census(*case) for name, case in R.SAMPLER_CASES().items()}


def test_sampler_reference_in_mode_first_is_the_oracle_sampler():
    """Mode first is ops_ref.sample with choose_first; in mode random the counts are the same and every index is a candidate."""
    checked = 0
    for name, (g, num, max_pos, mode, seed) in R.SAMPLER_CASES().items():
        if g.shape[1] > 20000:
            continue
        first = R.sample_reference(g, num, max_pos, 'first', seed)
        drawn = R.sample_reference(g, num, max_pos, 'random', seed)
        for b in range(g.shape[0]):
            gt = torch.from_numpy(g[b])
            pos = torch.nonzero(gt > 0).flatten()[:max_pos].numpy()
            neg = torch.nonzero(gt == 0).flatten()[:max(num - len(pos), 0)].numpy()
            if int(num * (max_pos / num)) == max_pos:            # (a fraction that gives max_pos back)
                checked += 1
                p2, n2 = ops_ref.sample(gt, num, max_pos / num)
                assert np.array_equal(p2.numpy(), pos) and np.array_equal(n2.numpy(), neg), (name, b)
            for c, want in ((0, pos), (1, neg)):
                k = len(want)
                assert np.array_equal(first[2 * c][b, :k], want), (name, b, c)
                for out in (first, drawn):
                    assert out[2 * c + 1][b].tolist() == [1] * k + [0] * (out[2 * c].shape[1] - k), (name, b, c)
                    assert (out[2 * c][b, k:] == g.shape[1] - 1).all(), (name, b, c)
                d = drawn[2 * c][b, :k]
                assert (np.diff(d) > 0).all() and ((g[b, d] > 0) if c == 0 else (g[b, d] == 0)).all(), (name, b, c)
    assert checked >= 30


def test_sampler_keys_known_answer():
    """splitmix64 of the published test vector: seed 1234567, first outputs 6457827717110365317, 3203168211198807973 (the sampler's
    key of index i is the high half of output i + 1 of the stream seeded with s)."""
    ks = R.sample_keys(0, 0, 0, np.arange(4))
    s = R.stream_seed(0, 0, 0)
    assert s == R.IMAGE_MIX and R.stream_seed(5, 1, 1) == ((5 ^ (2 * R.IMAGE_MIX % 2 ** 64)) + 1) % 2 ** 64

    def splitmix(state):
        z = (state + R.GOLDEN) % 2 ** 64
        x = z
        x = ((x ^ (x >> 30)) * R.MUL1) % 2 ** 64
        x = ((x ^ (x >> 27)) * R.MUL2) % 2 ** 64
        return z, x ^ (x >> 31)
    st, first = splitmix(1234567)
    _, second = splitmix(st)
    assert (first, second) == (6457827717110365317, 3203168211198807973)
    st = s
    for i in range(4):
        st, out = splitmix(st)
        assert int(ks[i]) == out >> 32


def test_sampler_census_reaches_every_path():
    census = _census()
    rows = [dict(r, case=n) for n, rs in census.items() for r in rs]
    by_path = collections.defaultdict(list)
    for r in rows:
        by_path[r['path']].append(r)
    print({p: (sum(r['c'] == 0 for r in by_path[p]), sum(r['c'] == 1 for r in by_path[p])) for p in R.PATHS})
    for p in R.PATHS:
        assert len(by_path[p]) >= 2, p
        assert {r['c'] for r in by_path[p]} == {0, 1}, p                 # positives and negatives on every path

    def has(path, **kw):
        pred = kw.pop('pred', lambda r: True)
        return any(all(r[k] == v for k, v in kw.items()) and pred(r) for r in by_path[path])
    # head of the pool: everything, nothing, mode first
    assert has(R.HEAD, pred=lambda r: r['k'] == r['cnt'] > 0) and has(R.HEAD, pred=lambda r: r['k'] == 0 < r['cnt'])
    assert any(r['path'] == R.HEAD and 0 < r['k'] < r['cnt'] for r in census['head_first_N3080'])
    # pooled select: k = 1, k = cnt - 1, cnt == 4096
    assert has(R.POOLED, k=1) and has(R.POOLED, pred=lambda r: r['k'] == r['cnt'] - 1 > 1) and has(R.POOLED, cnt=R.POOL)
    # pre-filter: the RPN's shape; k <= m <= 4096 on every such row, m > 4096 on every overflow row
    g, num, _, _, _ = R.SAMPLER_CASES()['prefilter_rpn']
    assert g.shape[1] == 261888 and num == 256 and sum(r['path'] == R.PREFILTER for r in census['prefilter_rpn']) >= 3
    assert all(r['k'] <= r['m'] <= R.POOL and r['cnt'] > 16 * r['k'] for r in by_path[R.PREFILTER])
    assert all(r['m'] > R.POOL for r in by_path[R.OVERFLOW])
    assert any(r['k'] == 1024 and r['cnt'] == 100000 for r in by_path[R.OVERFLOW])
    # full passes: cnt == 4097, cnt == 16k; cnt == 16k + 1 is the first count the pre-filter takes
    assert has(R.FULL, cnt=R.POOL + 1) and has(R.FULL, pred=lambda r: r['cnt'] == 16 * r['k'])
    assert has(R.PREFILTER, pred=lambda r: r['cnt'] == 16 * r['k'] + 1)
    assert all(R.POOL < r['cnt'] <= 16 * r['k'] for r in by_path[R.FULL])
    # general compaction: first / everything; the exit in the first of several rounds, and only in the last of three
    assert has(R.GENERAL, pred=lambda r: r['rounds'] > 1 and r['exit_round'] == 0 and r['k'] > 0)
    assert has(R.GENERAL, pred=lambda r: r['rounds'] >= 3 and r['exit_round'] == r['rounds'] - 1 and r['k'] == r['cnt'])
    assert has(R.GENERAL, pred=lambda r: r['rounds'] >= 3 and r['exit_round'] == r['rounds'] - 1 and r['k'] < r['cnt'])
    assert has(R.GENERAL, pred=lambda r: r['k'] == 0)


def test_sampler_census_reaches_every_edge():
    cases, census = R.SAMPLER_CASES(), _census()
    sizes = {c[0].shape[1] for c in cases.values()}
    assert {1, 15, 16, 17, 100, 3080, 16384, 16385} <= sizes
    assert any(c[0].shape[1] < c[1] for c in cases.values())                                    # N < num
    assert sum(c[0].shape[0] == 3 for c in cases.values()) >= 10
    rows = [r for rs in census.values() for r in rs]
    images = [(g[b], num, max_pos) for g, num, max_pos, _, _ in cases.values() for b in range(g.shape[0])]
    assert any((g > 0).sum() == 0 < (g == 0).sum() for g, _, _ in images) and any((g == 0).sum() == 0 < (g > 0).sum() for g, _, _ in images)
    assert any((g == -1).all() for g, _, _ in images)
    assert any(R.quotas(g, num, mp)[1] == num and R.quotas(g, num, mp)[2] > 0 for g, num, mp in images)     # negative quota 0
    # index N-1: a candidate that a random draw takes in one row and leaves in another -- for both classes
    for c in (0, 1):
        assert any(r['c'] == c and r['draws'] and r['last_is_candidate'] and r['last_drawn'] for r in rows), c
        assert any(r['c'] == c and r['draws'] and r['last_is_candidate'] and not r['last_drawn'] for r in rows), c
    # images with equal content draw differently (and image 2 of the first such row differs in content)
    for name in R.TWINS:
        g, num, max_pos, mode, seed = cases[name]
        assert np.array_equal(g[0], g[1]) and mode == 'random'
        ref = R.sample_reference(g, num, max_pos, mode, seed)
        assert not np.array_equal(ref[0][0], ref[0][1]) and not np.array_equal(ref[2][0], ref[2][1]), name
    assert any(not np.array_equal(g[0], g[-1]) for g, _, _, _, _ in cases.values())


def test_tie_seeds_tie():
    """The committed (seed, k) of every tie row is what the search finds from seed 1 on; the k-th and (k+1)-th smallest keys are equal
    and k - 1, k, k + 1 stay on the row's path."""
    paths = set()
    for name, spec in R.TIE_SPECS.items():
        seed, k = R.TIE_SEEDS[name]
        assert R.tie_search(spec, 1) == (seed, k), name
        cand = R.tie_candidates(spec)
        keys = np.sort(R.sample_keys(seed, 0, spec['cls'], cand))
        assert keys[k - 1] == keys[k] and keys[k - 2] < keys[k - 1] < keys[k + 1], name
        lo, hi = R.tie_pair(name)
        assert lo < hi
        for kk, both in ((k - 1, (False, False)), (k, (True, False)), (k + 1, (True, True))):
            case = R.tie_case(name, kk)
            row = R.sample_census(*case)[spec['cls']]
            assert row['path'] == spec['path'] and row['k'] == kk and row['cnt'] == spec['cnt'], (name, kk, row)
            took = R.sample_reference(*case)[2 * spec['cls']][0, :kk]
            assert (lo in took, hi in took) == both, (name, kk)
        paths.add(spec['path'])
    assert {R.POOLED, R.PREFILTER} <= paths and paths & {R.OVERFLOW, R.FULL}


def test_sampler_draws_are_uniform():
    """N = 64, k = 16, seeds 0 .. 3999: every index is included T/4 times within 5 sigma (binomial), for both classes and for image 0
    and image 1; the positive and the negative draw of one seed over the same 64 candidates overlap like independent draws do
    (hypergeometric: mean k^2/N = 4 per seed, variance k (k/N) (1 - k/N) (N - k)/(N - 1) = 16/7)."""
    T, N, k = R.UNI_T, R.UNI_N, R.UNI_K
    p = k / N
    bound = 5 * np.sqrt(T * p * (1 - p))
    took = [R.uniform_draws(c) for c in (0, 1)]
    for c in (0, 1):
        for b in (0, 1):
            counts = took[c][b].sum(0)
            print(c, b, int(counts.min()), int(counts.max()), 'bound', T * p - bound, T * p + bound)
            assert (np.abs(counts - T * p) <= bound).all(), (c, b, counts)
    var = k * p * (1 - p) * (N - k) / (N - 1)
    for b in (0, 1):
        overlap = int((took[0][b] & took[1][b]).sum())
        print('overlap', b, overlap, 'expected', T * k * p, '+-', 5 * np.sqrt(T * var))
        assert abs(overlap - T * k * p) <= 5 * np.sqrt(T * var), (b, overlap)
    overlap = int((took[0][0] & took[0][1]).sum())                    # image 0 against image 1, same class, same seed
    assert abs(overlap - T * k * p) <= 5 * np.sqrt(T * var), overlap


# ---- assigner --------------------------------------------------------------------------------------------------------------------
def test_assigner_reference_is_the_oracle_assigner():
    """Every image of every scene under every form: gt_inds equal, max_overlaps equal bit for bit."""
    for name, sc in R.ASSIGNER_SCENES().items():
        for thr, lq in R.FORMS:
            gi, mo = R.scene_reference(sc, thr, lq)
            for b in range(sc['boxes'].shape[0]):
                nb, ng = int(sc['nbox'][b]), int(sc['ngt'][b])
                want_gi, want_mo = ops_ref.max_iou_assign(torch.from_numpy(sc['boxes'][b, :nb]), torch.from_numpy(sc['gts'][b, :ng]),
                                                          thr[0], thr[1], thr[2], lq)
                assert np.array_equal(gi[b, :nb], want_gi.numpy()) and (gi[b, nb:] == -1).all(), (name, thr, lq, b)
                assert np.array_equal(mo[b].view(np.int32), want_mo.numpy().view(np.int32)), (name, thr, lq, b)
                assert not np.isnan(mo[b]).any()


def test_assigner_scenes_cover_sizes_forms_and_padding():
    scenes = R.ASSIGNER_SCENES()
    assert {(s['boxes'].shape[1], s['gts'].shape[1]) for n, s in scenes.items() if n.startswith('size_')} == {(n, k) for n in R.NMAX for k in R.KMAX}
    assert all(s['boxes'].shape[1] <= 1100 and s['boxes'].shape[0] == 3 for s in scenes.values())
    forms = set(R.FORMS)
    assert {(t[2] > 0, lq) for t, lq in forms} == {(True, True), (False, True), (True, False), (False, False)}
    assert {t for t, _ in forms} == {(0.7, 0.3, 0.3), (0.5, 0.5, 0.5), (0.5, 0.25, 0.25), (0.5, 0.5, 0.0)}
    nan = cover = 0
    for s in scenes.values():
        for b in range(3):
            rest = np.concatenate([s['boxes'][b, s['nbox'][b]:].ravel(), s['gts'][b, s['ngt'][b]:].ravel()])
            nan += int(rest.size and np.isnan(rest).all())
            cover += int(rest.size and (np.abs(rest) == 1e4).all())
            assert not np.isnan(s['boxes'][b, :s['nbox'][b]]).any() and not np.isnan(s['gts'][b, :s['ngt'][b]]).any()
    assert nan >= 10 and cover >= 10
    total = collections.Counter()
    for s in scenes.values():
        total.update(R.scene_census(s))
    print(dict(total))
    assert total['ends_in_wave'] >= 10 and total['no_gt'] >= 10


def test_assigner_geometry_census():
    """The hand-placed scene holds every situation by construction; the census finds them, and the reference resolves them as
    MaxIoUAssigner must."""
    sc = R.geometry_scene('cover')
    c = R.scene_census(sc)
    print(c)
    for key in ('shared_max', 'dup_gt', 'later_block_only', 'two_blocks', 'touching', 'empty_box', 'empty_gt', 'two_unmatched', 'ends_in_wave'):
        assert c[key] > 0, key
    half = R.threshold_census(sc, (0.5, 0.5, 0.5))
    quarter = R.threshold_census(sc, (0.5, 0.25, 0.25))
    print(half, quarter)
    for t in (half, quarter):                        # each comparison meets its threshold exactly, and misses it on either side
        assert all(t[k] > 0 for k in t), t
    ov = R.iou_matrix(sc['gts'][0, :sc['ngt'][0]], sc['boxes'][0])
    assert ov[0, 3] == 1 and ov[0, 4] == 0.5 and ov[0, 5] == 0.25 and ov[0, 6] == 0.125 and ov[10, 21] == np.float32(1) / np.float32(7)
    # (0.5, 0.25, 0.25) without low-quality matching: 0.5 is positive, 0.25 is not negative, 0.125 is
    gi, _ = R.scene_reference(sc, (0.5, 0.25, 0.25), False)
    assert gi[0, 3] == 1 and gi[0, 4] == 1 and gi[0, 5] == -1 and gi[0, 6] == 0
    assert gi[0, 7] == -1 and gi[0, 15] == 7 and gi[0, 12] == gi[0, 13] == gi[0, 270] == 6
    # ... with it: the gt whose maximum is exactly min_pos takes its box; the later of two equal gts takes theirs; all copies of a maximum
    gi, _ = R.scene_reference(sc, (0.5, 0.25, 0.25), True)
    assert gi[0, 7] == 3 and gi[0, 15] == 8 and gi[0, 16] == 7 and gi[0, 530] == 9 and gi[0, 10] == gi[0, 300] == 10
    gi, _ = R.scene_reference(sc, (0.7, 0.3, 0.3), True)
    assert gi[0, 12] == gi[0, 13] == gi[0, 270] == 6 and gi[0, 14] == 0
    # min_pos == 0: gts 1, 3 and 11 overlap nothing; the last of them takes every box that no later gt claims
    gi, _ = R.scene_reference(sc, (0.5, 0.5, 0.0), True)
    assert gi[0, 100] == 12 and gi[0, 5] == 12 and gi[0, 599] == 13 and gi[0, 22] == 12
    assert gi[2, 100] == 4 and (gi[2, 560:] == -1).all()
    gi, _ = R.scene_reference(sc, (0.5, 0.5, 0.0), False)
    assert gi[0, 100] == 0 and gi[0, 5] == 0


def test_assigner_strip_census():
    """Anchor-like boxes: gts outside some runs of 64 boxes and inside others, one exactly tangent to a run's bounding box, and one that
    only the second half of a run overlaps (a bounding box over 32 lanes would lose it)."""
    for name in ('anchors', 'anchors_cover'):
        c = R.strip_census(R.ASSIGNER_SCENES()[name])
        print(name, c)
        assert c['outside'] > 0 and c['inside'] > 0 and c['tangent'] > 0 and c['half'] > 0, c
    sc = R.ASSIGNER_SCENES()['anchors']
    gi, mo = R.scene_reference(sc, (0.7, 0.3, 0.3), True)
    assert (gi[0] > 0).sum() >= sc['ngt'][0] - 1 and (mo[0] > 0).any()
