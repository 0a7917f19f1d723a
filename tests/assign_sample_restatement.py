"""Plain numpy statements of the two selection kernels of csrc/boxes.hip -- loft_iou_assign (MaxIoUAssigner) and loft_random_sample
(RandomSampler on hashed keys) -- with the case tables of tests/test_assign_sample_{cpu,gpu}.py and the censuses that say which
kernel path each case reaches.

The references are written from the contract, not from the kernels: the sampler is one stable argsort of (key, index) per class, the
assigner is the whole K x N IoU matrix in float32 followed by max / argmax / thresholds / the sequential per-gt loop.  Only the
censuses restate anything of the kernels, and only their dispatch rules (which of the selection paths a candidate count and a quota
reach; which gts lie outside the bounding box of a run of 64 boxes)."""
import numpy as np

# ======================================================================================================================= sampler
MASK64 = (1 << 64) - 1
IMAGE_MIX = 0xD6E8FEB86659FD93
GOLDEN = 0x9E3779B97F4A7C15
MUL1, MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
POOL = 4096                  # candidates the kernel keeps on chip
ROUND = 16384                # boxes per round of its ordered compaction


def stream_seed(seed, b, c):
    """Seed of image b's class c (0: positives, 1: negatives)."""
    return (((seed & MASK64) ^ (((b + 1) * IMAGE_MIX) & MASK64)) + c) & MASK64


def sample_keys(seed, b, c, idx):
    """uint32 key of every index in `idx`: high half of the splitmix64 finaliser of s + (i + 1) * GOLDEN."""
    with np.errstate(over='ignore'):
        z = np.uint64(stream_seed(seed, b, c)) + (np.asarray(idx).astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MUL2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def quotas(gt_row, num, max_pos):
    """(#pos, k_pos, #neg, k_neg) of one image."""
    n = gt_row.shape[0]
    npos, nneg = int((gt_row > 0).sum()), int((gt_row == 0).sum())
    k_pos = min(npos, min(max_pos, n))
    k_neg = min(nneg, max(num - k_pos, 0), min(num, n))
    return npos, k_pos, nneg, k_neg


def choose(cand, k, mode, seed, b, c):
    """The k chosen of the candidates `cand` (ascending indices), ascending."""
    if mode == 'first' or k == cand.shape[0]:
        return cand[:k]
    keys = sample_keys(seed, b, c, cand)
    order = np.argsort(keys, kind='stable')              # (key, index): cand is ascending
    return np.sort(cand[order[:k]])


def sample_reference(gt_inds, num, max_pos, mode, seed):
    """gt_inds int64 [B, N] -> (pos_idx int64 [B,P], pos_valid uint8 [B,P], neg_idx [B,Q], neg_valid [B,Q])."""
    B, N = gt_inds.shape
    P, Q = min(max_pos, N), min(num, N)
    out = [np.full((B, P), N - 1, np.int64), np.zeros((B, P), np.uint8), np.full((B, Q), N - 1, np.int64), np.zeros((B, Q), np.uint8)]
    for b in range(B):
        _, k_pos, _, k_neg = quotas(gt_inds[b], num, max_pos)
        for c, k in ((0, k_pos), (1, k_neg)):
            cand = np.flatnonzero(gt_inds[b] > 0 if c == 0 else gt_inds[b] == 0)
            out[2 * c][b, :k] = choose(cand, k, mode, seed, b, c)
            out[2 * c + 1][b, :k] = 1
    return tuple(out)


# ---- census: the kernel's dispatch rule, and nothing else of it
HEAD, POOLED, PREFILTER, OVERFLOW, FULL, GENERAL = 'head of pool', 'pooled select', 'pre-filter then pooled', \
    'pre-filter overflow into the full passes', 'full passes without a pre-filter', 'general compaction'
PATHS = (HEAD, POOLED, PREFILTER, OVERFLOW, FULL, GENERAL)


def survivors(keys, cnt, k):
    """How many keys lie below the pre-filter's cut floor(8k / cnt * 2^32), the cut computed in double."""
    cut = 8.0 * float(k) / float(cnt) * 4294967296.0
    t0 = 0xffffffff if cut >= 4294967295.0 else int(cut)
    return int((keys < np.uint32(t0)).sum())


def sample_path(cnt, k, mode, m):
    """Path of one (image, class): cnt candidates, k to take, m survivors of the pre-filter (used only where it runs)."""
    draw = mode == 'random' and 0 < k < cnt
    if cnt <= POOL:
        return POOLED if draw else HEAD
    if not draw:
        return GENERAL
    if cnt > 16 * k:
        return PREFILTER if k <= m <= POOL else OVERFLOW
    return FULL


def sample_census(gt_inds, num, max_pos, mode, seed):
    """One dict per (image, class): path, cnt, k, m, whether index N-1 is a candidate / is drawn, and for the general compaction the
    round (of ROUND boxes) in which its early exit fires and the number of rounds."""
    B, N = gt_inds.shape
    ref = sample_reference(gt_inds, num, max_pos, mode, seed)
    rows = []
    for b in range(B):
        npos, k_pos, nneg, k_neg = quotas(gt_inds[b], num, max_pos)
        for c, cnt, k in ((0, npos, k_pos), (1, nneg, k_neg)):
            cand = np.flatnonzero(gt_inds[b] > 0 if c == 0 else gt_inds[b] == 0)
            m = -1
            if mode == 'random' and 0 < k < cnt and cnt > POOL and cnt > 16 * k:
                m = survivors(sample_keys(seed, b, c, cand), cnt, k)
            path = sample_path(cnt, k, mode, m)
            row = dict(b=b, c=c, cnt=cnt, k=k, m=m, path=path, last_is_candidate=bool(cnt and cand[-1] == N - 1),
                       last_drawn=bool(k and ref[2 * c][b, k - 1] == N - 1), draws=mode == 'random' and 0 < k < cnt)
            if path == GENERAL:
                row['rounds'] = -(-N // ROUND)
                row['exit_round'] = int(cand[k - 1]) // ROUND if k else 0
            rows.append(row)
    return rows


def layout(N, npos, nneg, seed, last=None, span=None):
    """int64 [N]: npos positives (values 1..80) and nneg negatives at random places, the rest ignored (-1).  last: class of index N-1
    ('pos', 'neg', 'ign'; None: as it falls).  span: (lo, hi) keeps every candidate inside [lo, hi)."""
    rng = np.random.RandomState(seed)
    lo, hi = span if span else (0, N)
    free = hi - lo - (1 if last and hi == N else 0)
    kp, kn = npos - (last == 'pos'), nneg - (last == 'neg')
    assert 0 <= kp and 0 <= kn and kp + kn <= free, (N, npos, nneg, last, span)
    place = lo + rng.permutation(free)[:kp + kn]
    g = np.full(N, -1, np.int64)
    g[place[:kp]] = rng.randint(1, 81, size=kp)
    g[place[kp:]] = 0
    if last == 'pos':
        g[N - 1] = 7
    elif last == 'neg':
        g[N - 1] = 0
    assert int((g > 0).sum()) == npos and int((g == 0).sum()) == nneg
    return g


def _stack(*rows):
    return np.stack(rows)


def sampler_cases():
    """name -> (gt_inds [B,N], num, max_pos, mode, seed).  Built once (see SAMPLER_CASES)."""
    c = {}
    # ---- head of the pool: everything taken, nothing taken, mode first; N < num; no positives / no negatives / all ignored
    c['head_all_N100'] = (_stack(layout(100, 10, 50, 1, last='neg'), layout(100, 0, 100, 2), layout(100, 100, 0, 3)), 256, 64, 'random', 11)
    c['head_all_ignored'] = (_stack(np.full(100, -1, np.int64), layout(100, 7, 0, 4, last='pos'), layout(100, 0, 9, 5, last='ign')),
                             16, 4, 'random', 12)
    c['head_first_N3080'] = (_stack(layout(3080, 200, 2500, 6), layout(3080, 30, 3000, 7, last='pos'), layout(3080, 2000, 1000, 8, last='neg')),
                             256, 64, 'first', 13)
    c['quota_zero_N3080'] = (_stack(layout(3080, 600, 2000, 9), layout(3080, 512, 2568, 10), layout(3080, 3080, 0, 11)), 512, 512, 'random', 14)
    # ---- pooled select: k = 1, k = cnt - 1, cnt == 4096, the small N of the 16-byte tail
    c['pooled_k1_N17'] = (_stack(layout(17, 5, 10, 12, last='neg'), layout(17, 8, 9, 13, last='pos'), layout(17, 2, 2, 14)), 2, 1, 'random', 15)
    c['pooled_kcnt1_N100'] = (_stack(layout(100, 33, 60, 15, last='pos'), layout(100, 33, 60, 16, last='neg'), layout(100, 33, 67, 17)),
                              91, 32, 'random', 16)
    c['pooled_4096_N16384'] = (_stack(layout(16384, 4096, 4096, 18, last='neg'), layout(16384, 4096, 12288, 19, last='pos'),
                                      layout(16384, 4095, 4096, 20)), 512, 128, 'random', 17)
    for n in (1, 15, 16):
        c[f'small_N{n}'] = (_stack(layout(n, n // 2, n - n // 2, 21 + n, last='neg'), layout(n, n - n // 2, n // 2, 22 + n, last='pos'),
                                   layout(n, n // 3, n // 3, 23 + n)), 4, 2, 'random', 18 + n)
    c['pooled_N3080_rcnn'] = (_stack(layout(3080, 300, 2700, 40, last='neg'), layout(3080, 100, 2900, 41, last='pos'), layout(3080, 1500, 1500, 42)),
                              512, 128, 'random', 40)
    # ---- pre-filter then pooled: the RPN's shape, both classes above 16k
    c['prefilter_rpn'] = (_stack(layout(261888, 300, 250000, 43, last='neg'), layout(261888, 120000, 120000, 44, last='pos'),
                                 layout(261888, 5, 261883, 45)), 256, 128, 'random', 41)
    c['boundary_16k_N16385'] = (_stack(layout(16385, 4800, 4801, 46, last='pos'), layout(16385, 4801, 4800, 47, last='neg')), 600, 300, 'random', 42)
    # ---- pre-filter overflow: 8k survivors expected, 4096 fit
    c['overflow_num2048'] = (_stack(layout(200000, 100000, 100000, 48, last='neg'), layout(200000, 90000, 100000, 49, last='pos')),
                             2048, 1024, 'random', 43)
    c['overflow_num2048_p600'] = (_stack(layout(150001, 50000, 100000, 50), layout(150001, 30000, 110000, 51, last='neg')), 2048, 600, 'random', 44)
    # ---- full passes without a pre-filter: 4096 < cnt <= 16k, at cnt == 4097 and cnt == 16k
    c['full_4097_N16385'] = (_stack(layout(16385, 4097, 4097, 52, last='neg'), layout(16385, 4097, 8000, 53, last='pos')), 1024, 512, 'random', 45)
    c['full_mid_N16384'] = (_stack(layout(16384, 6000, 10000, 54, last='pos'), layout(16384, 5000, 11000, 55, last='neg')), 4000, 2000, 'random', 46)
    # ---- general compaction: early exit in the first round; only in the last of three rounds
    c['general_first_round'] = (_stack(layout(50000, 5000, 9000, 56, span=(0, 16000)), layout(50000, 6000, 8000, 57, span=(100, 16384))),
                                256, 128, 'first', 47)
    c['general_all_last_round'] = (_stack(layout(40000, 5000, 30000, 58, last='pos'), layout(40000, 8000, 32000, 59, last='neg')),
                                   50000, 6000, 'random', 48)
    c['general_first_last_round'] = (_stack(layout(40000, 5000, 30000, 60, last='pos'), layout(40000, 6000, 30000, 61, last='neg')),
                                     34998, 4999, 'first', 49)
    c['general_quota_zero'] = (_stack(layout(20000, 6000, 10000, 65), layout(20000, 512, 19000, 66, last='neg')), 512, 512, 'random', 52)
    # ---- two images with the same gt_inds: different draws
    twin = layout(3080, 400, 2600, 62)
    c['twins_N3080'] = (_stack(twin, twin, layout(3080, 400, 2600, 63)), 512, 128, 'random', 50)
    twin = layout(100000, 20000, 80000, 64)
    c['twins_N100000'] = (_stack(twin, twin), 256, 64, 'random', 51)
    return c


_SAMPLER_CASES = []


def SAMPLER_CASES():
    if not _SAMPLER_CASES:
        _SAMPLER_CASES.append(sampler_cases())
    return _SAMPLER_CASES[0]


TWINS = ('twins_N3080', 'twins_N100000')

# ---- ties at the threshold.  One image of N boxes with cnt candidates of class cls; a seed is wanted under which the k-th and the
# (k + 1)-th smallest keys are equal for some k in [k_lo, k_hi], the range in which k - 1, k and k + 1 all take `path`.
TIE_SPECS = {
    'tie_pooled_pos': dict(N=16384, cnt=4096, cls=0, layout_seed=70, k_lo=2, k_hi=4094, path=POOLED),
    'tie_prefilter_neg': dict(N=261888, cnt=261888, cls=1, layout_seed=71, k_lo=17, k_hi=479, path=PREFILTER),
    'tie_overflow_pos': dict(N=110000, cnt=100000, cls=0, layout_seed=72, k_lo=700, k_hi=6000, path=OVERFLOW),
    'tie_full_neg': dict(N=16384, cnt=16000, cls=1, layout_seed=73, k_lo=1100, k_hi=15998, path=FULL),
}
# name -> (seed, k): what tie_search(spec, 1) returns (0.3 s for all four); tests/test_assign_sample_cpu.py derives them again
TIE_SEEDS = {'tie_pooled_pos': (510, 1836), 'tie_prefilter_neg': (31, 21), 'tie_overflow_pos': (12, 1833), 'tie_full_neg': (31, 2966)}


def tie_layout(spec):
    if spec['cls'] == 0:
        return layout(spec['N'], spec['cnt'], spec['N'] - spec['cnt'], spec['layout_seed'])
    return layout(spec['N'], 0, spec['cnt'], spec['layout_seed'])


def tie_candidates(spec):
    g = tie_layout(spec)
    return np.flatnonzero(g > 0 if spec['cls'] == 0 else g == 0)


def tie_at(spec, seed, cand=None):
    """The smallest k in [k_lo, k_hi] whose k-th and (k+1)-th smallest keys (image 0) are equal under `seed`, or 0."""
    cand = tie_candidates(spec) if cand is None else cand
    keys = np.sort(sample_keys(seed, 0, spec['cls'], cand))
    eq = np.flatnonzero(keys[1:] == keys[:-1]) + 1           # 1-based rank of the first of an equal pair
    eq = eq[(eq >= spec['k_lo']) & (eq <= spec['k_hi'])]
    return int(eq[0]) if eq.size else 0


def tie_search(spec, first=1, tries=20000):
    """(seed, k): the first seed from `first` on with such a tie."""
    cand = tie_candidates(spec)
    for seed in range(first, first + tries):
        k = tie_at(spec, seed, cand)
        if k:
            return seed, k
    raise LookupError('no tie within %d seeds' % tries)


def tie_case(name, k):
    """(gt_inds [1,N], num, max_pos, 'random', seed) that asks image 0's tie class for exactly k."""
    spec = TIE_SPECS[name]
    g = tie_layout(spec)[None]
    seed = TIE_SEEDS[name][0]
    return (g, k, k, 'random', seed) if spec['cls'] == 0 else (g, k, 0, 'random', seed)


def tie_pair(name):
    """Indices (lower, higher) of the two candidates that share the k-th smallest key."""
    spec = TIE_SPECS[name]
    seed, k = TIE_SEEDS[name]
    cand = tie_candidates(spec)
    keys = sample_keys(seed, 0, spec['cls'], cand)
    order = np.argsort(keys, kind='stable')
    assert keys[order[k - 1]] == keys[order[k]]
    return int(cand[order[k - 1]]), int(cand[order[k]])


# ---- uniformity of the reference's draws (the kernel equals the reference bit for bit)
UNI_N, UNI_K, UNI_T = 64, 16, 4000


def uniform_draws(c):
    """bool [2, T, N]: whether image b's class-c draw of seed t (seeds 0 .. UNI_T-1) holds candidate i; every index is a candidate."""
    g = np.full((2, UNI_N), 1 if c == 0 else 0, np.int64)
    took = np.zeros((2, UNI_T, UNI_N), bool)
    for seed in range(UNI_T):
        out = sample_reference(g, UNI_K, UNI_K if c == 0 else 0, 'random', seed)
        assert out[2 * c + 1].all() and out[2 * c].shape == (2, UNI_K)
        for b in range(2):
            took[b, seed, out[2 * c][b]] = True
    return took


# ====================================================================================================================== assigner
F32 = np.float32
THRESHOLDS = ((0.7, 0.3, 0.3), (0.5, 0.5, 0.5), (0.5, 0.25, 0.25), (0.5, 0.5, 0.0))       # (pos, neg, min_pos)
FORMS = tuple((thr, lq) for thr in THRESHOLDS for lq in (True, False))
NMAX = (1, 63, 64, 65, 255, 256, 257, 1030)
KMAX = (0, 1, 2, 80)
WAVE, BLOCK = 64, 256


def iou_matrix(gts, boxes):
    """float32 [K, N], one rounded operation after the other (no fused multiply-add: numpy has none)."""
    g, b = gts.astype(F32)[:, None, :], boxes.astype(F32)[None, :, :]
    ltx, lty = np.maximum(g[..., 0], b[..., 0]), np.maximum(g[..., 1], b[..., 1])
    rbx, rby = np.minimum(g[..., 2], b[..., 2]), np.minimum(g[..., 3], b[..., 3])
    w, h = np.maximum(rbx - ltx, F32(0)), np.maximum(rby - lty, F32(0))
    overlap = w * h
    a1 = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    a2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    union = np.maximum(a1 + a2 - overlap, F32(1e-6))
    out = overlap / union
    assert out.dtype == F32
    return out


def assign_reference(boxes, gts, pos_thr, neg_thr, min_pos, low_quality):
    """MaxIoUAssigner: boxes [N,4], gts [K,4] -> (gt_inds int64 [N]: -1 ignored, 0 negative, i + 1 positive; max_ov float32 [N])."""
    n, k = boxes.shape[0], gts.shape[0]
    if k == 0 or n == 0:
        return np.full(n, 0 if k == 0 else -1, np.int64), np.zeros(n, F32)
    ov = iou_matrix(gts, boxes)
    max_ov, arg = ov.max(0), ov.argmax(0)                    # argmax: the first of equal maxima
    gt_max = ov.max(1)
    gt_inds = np.full(n, -1, np.int64)
    gt_inds[(max_ov >= F32(0)) & (max_ov < F32(neg_thr))] = 0
    pos = max_ov >= F32(pos_thr)
    gt_inds[pos] = arg[pos] + 1
    if low_quality:
        for i in range(k):                                   # in order: a later gt takes the box from an earlier one
            if gt_max[i] >= F32(min_pos):
                gt_inds[ov[i] == gt_max[i]] = i + 1
    return gt_inds, max_ov


def lattice_boxes(rng, n, size=12):
    """Half of them on an integer lattice (equal IoUs, IoUs on a threshold, shared edges and empty boxes are common), half anywhere."""
    a = rng.randint(0, size, size=(n, 2)).astype(F32)
    wh = rng.randint(0, 5, size=(n, 2)).astype(F32)
    free = rng.rand(n) < 0.5
    a = np.where(free[:, None], (rng.rand(n, 2) * size).astype(F32), a)
    wh = np.where(free[:, None], (rng.rand(n, 2) * 5 + 0.05).astype(F32), wh)
    return np.concatenate([a, a + wh], 1).astype(F32)


def _scene(boxes, nbox, gts, ngt, pad):
    """Padded float32 [B,Nmax,4] / [B,Kmax,4]: rows at or beyond nbox / ngt hold `pad` ('nan' or 'cover')."""
    boxes, gts = np.array(boxes, F32), np.array(gts, F32)
    fill = np.array([np.nan] * 4 if pad == 'nan' else [-1e4, -1e4, 1e4, 1e4], F32)
    for b in range(boxes.shape[0]):
        boxes[b, nbox[b]:] = fill
        gts[b, ngt[b]:] = fill
    return dict(boxes=boxes, nbox=np.array(nbox, np.int32), gts=gts, ngt=np.array(ngt, np.int32))


def size_scene(nmax, kmax, pad='nan'):
    """B = 3, ragged: image 0 full; image 1 ends inside a wavefront, one gt fewer; image 2 has no gt."""
    rng = np.random.RandomState(1000 * kmax + nmax)
    boxes = np.stack([lattice_boxes(rng, nmax) for _ in range(3)])
    gts = np.stack([lattice_boxes(rng, kmax) for _ in range(3)]).reshape(3, kmax, 4)
    for b in range(2):                                       # exact matches and a repeated box, as far as they fit
        m = min(kmax, nmax) // 2
        boxes[b, :m] = gts[b, :m]
        if nmax > 40:
            boxes[b, 37] = boxes[b, 5]
    nbox = [nmax, nmax - nmax // 3, max(nmax - 1, 0)]
    ngt = [kmax, max(kmax - 1, 0), 0]
    return _scene(boxes, nbox, gts, ngt, pad)


def geometry_scene(pad='cover', order=0):
    """Hand-placed motifs, each in its own 32 x 32 cell of the plane (coordinates are small integers: every IoU below is exact), among
    lattice filler inside cell (0, 0).  B = 3: image 1 lists the gts in reverse, image 2 drops the last three gts and 40 boxes."""
    rng = np.random.RandomState(77)
    nmax = 600

    def at(cell, box):
        ox, oy = 32.0 * (cell % 8 + 1), 32.0 * (cell // 8 + 1)
        return [box[0] + ox, box[1] + oy, box[2] + ox, box[3] + oy]

    gts, put = [], {}
    # 0: IoU 1, 0.5, 0.25 and 0.125 against one gt -- both thresholds met exactly, by boxes that are NOT the gt's maximum
    gts.append(at(0, [0, 0, 1, 1]))
    put[3], put[4], put[5], put[6] = at(0, [0, 0, 1, 1]), at(0, [0, 0, 2, 1]), at(0, [0, 0, 4, 1]), at(0, [0, 0, 8, 1])
    # 1: a gt that overlaps nothing -- and (3) a later one, neither of them last
    gts.append(at(1, [0, 0, 3, 3]))
    # 2: a gt whose maximum is exactly 0.25
    gts.append(at(2, [0, 0, 1, 1]))
    put[7], put[8] = at(2, [0, 0, 4, 1]), at(2, [0, 0, 8, 1])
    gts.append(at(3, [0, 0, 2, 5]))
    # 4: a gt whose maximum is exactly 0.5
    gts.append(at(4, [0, 0, 1, 1]))
    put[9], put[11] = at(4, [0, 0, 2, 1]), at(4, [0, 0, 1, 4])
    # 5: three copies of the box that is the gt's maximum (0.5): all of them get it
    gts.append(at(5, [0, 0, 4, 4]))
    put[12] = put[13] = put[270] = at(5, [0, 0, 4, 2])
    put[14] = at(5, [0, 0, 4, 1])
    # 6, 7: the same gt twice; an identical box (argmax: the first; low quality: the last) and a box at IoU 2/3
    gts.append(at(6, [0, 0, 3, 3]))
    gts.append(at(6, [0, 0, 3, 3]))
    put[15], put[16] = at(6, [0, 0, 3, 3]), at(6, [0, 0, 3, 2])
    # 8: a gt whose maximum (0.5) is reached only in the third block; 9: one whose maximum is reached in the first and the second
    gts.append(at(8, [0, 0, 2, 2]))
    put[530], put[17] = at(8, [0, 0, 2, 1]), at(8, [0, 0, 8, 8])
    gts.append(at(9, [0, 0, 2, 4]))
    put[10], put[300] = at(9, [0, 0, 2, 3]), at(9, [0, 0, 2, 3])
    # 10: a box sharing an edge, a box sharing a corner, an empty box inside and a partial overlap (1/7)
    gts.append(at(10, [0, 0, 2, 2]))
    put[18], put[19], put[20], put[21] = at(10, [2, 0, 4, 2]), at(10, [2, 2, 4, 4]), at(10, [1, 1, 1, 1]), at(10, [1, 1, 3, 3])
    # 11: an empty gt under a box that covers it (it overlaps nothing); 12: a gt met exactly by the last box, in the last wavefront
    gts.append(at(11, [5, 5, 5, 5]))
    put[22] = at(11, [4, 4, 6, 6])
    gts.append(at(12, [0, 0, 5, 2]))
    put[599] = at(12, [0, 0, 5, 2])
    gts = np.array(gts, F32)
    k = gts.shape[0]
    boxes = lattice_boxes(rng, nmax)
    for i, bx in put.items():
        boxes[i] = bx
    fill = lattice_boxes(rng, 8)
    allg = np.stack([gts, gts[::-1], gts])
    allb = np.stack([boxes, boxes, boxes])
    allb[2, 40:48] = fill
    if order:
        allg = allg[:, ::-1]
    return _scene(allb, [nmax, nmax, nmax - 40], allg, [k, k, k - 3], pad)


def anchor_scene(pad='nan'):
    """Boxes enumerated like anchors (position-major over an 18 x 18 grid of stride 8, three shapes per position: 972 boxes, 16
    wavefronts) and gts placed against the strips: small ones inside a single strip, one touching a strip's bounding box from
    outside, one spanning every strip."""
    g = 18
    shapes = [(16, 16), (22, 12), (12, 22)]
    boxes = np.array([[8 * x + 4 - w / 2, 8 * y + 4 - h / 2, 8 * x + 4 + w / 2, 8 * y + 4 + h / 2]
                      for y in range(g) for x in range(g) for (w, h) in shapes], F32)
    n = boxes.shape[0]
    strips = strip_boxes(boxes, n)
    gts = [[40, 0, 52, 10],                                   # inside the first strips only
           [100, 0, 112, 10],                                 # overlaps the first run's boxes 32..63 only, outside the bbox of 0..31
           [0, 100, 30, 120],
           [100, 60, 112, 76],
           [0, strips[5][3], 20, strips[5][3] + 6],            # its top edge on the bottom edge of strip 5's bounding box
           [30, strips[9][1] - 5, 50, strips[9][1]],           # its bottom edge on the top edge of strip 9's
           [-20, -20, 170, 170],                              # every strip
           [60, 130, 61, 131]]                                # a small one inside the last strips
    gts = np.array(gts, F32)
    rng = np.random.RandomState(5)
    b1 = boxes + rng.randint(-2, 3, size=boxes.shape).astype(F32) * np.array([1, 1, 0, 0], F32)
    allb = np.stack([boxes, b1, boxes])
    allg = np.stack([gts, gts[::-1], gts])
    return _scene(allb, [n, n - 100, n - 33], allg, [len(gts), len(gts), 2], pad)


def strip_boxes(boxes, nbox):
    """[x1, y1, x2, y2] of every run of 64 consecutive boxes below nbox."""
    return [[boxes[s:min(s + WAVE, nbox), 0].min(), boxes[s:min(s + WAVE, nbox), 1].min(), boxes[s:min(s + WAVE, nbox), 2].max(),
             boxes[s:min(s + WAVE, nbox), 3].max()] for s in range(0, nbox, WAVE)]


def strip_census(scene):
    """Over every (run of 64 boxes, gt) of the scene: pairs outside (the gt cannot overlap any box of the run:
    g.x2 <= x1 | g.x1 >= x2 | g.y2 <= y1 | g.y1 >= y2), pairs inside, pairs tangent (outside, with equality), and pairs `half`: the gt
    overlaps a box among the run's last 32 and lies outside the bounding box of its first 32."""
    c = dict(outside=0, inside=0, tangent=0, half=0)
    for b in range(scene['boxes'].shape[0]):
        nb, ng = int(scene['nbox'][b]), int(scene['ngt'][b])
        boxes = scene['boxes'][b]
        for w, (x1, y1, x2, y2) in enumerate(strip_boxes(boxes, nb)):
            lo, mid, hi = w * WAVE, min(w * WAVE + 32, nb), min(w * WAVE + WAVE, nb)
            hx1, hy1, hx2, hy2 = boxes[lo:mid, 0].min(), boxes[lo:mid, 1].min(), boxes[lo:mid, 2].max(), boxes[lo:mid, 3].max()
            for g in scene['gts'][b, :ng]:
                outside = g[2] <= x1 or g[0] >= x2 or g[3] <= y1 or g[1] >= y2
                strictly = g[2] < x1 or g[0] > x2 or g[3] < y1 or g[1] > y2
                c['outside'] += int(outside)
                c['inside'] += int(not outside)
                c['tangent'] += int(outside and not strictly)
                if hi > mid and (g[2] <= hx1 or g[0] >= hx2 or g[3] <= hy1 or g[1] >= hy2):
                    c['half'] += int((iou_matrix(g[None], boxes[mid:hi]) > 0).any())
    return c


def assigner_scenes():
    """name -> scene.  Every scene runs under every form of FORMS."""
    s = {f'size_N{n}_K{k}': size_scene(n, k, 'nan' if (n + k) % 2 else 'cover') for n in NMAX for k in KMAX}
    s['geometry'] = geometry_scene('cover')
    s['geometry_nan_reversed'] = geometry_scene('nan', order=1)
    s['anchors'] = anchor_scene('nan')
    s['anchors_cover'] = anchor_scene('cover')
    return s


_ASSIGNER_SCENES = []


def ASSIGNER_SCENES():
    if not _ASSIGNER_SCENES:
        _ASSIGNER_SCENES.append(assigner_scenes())
    return _ASSIGNER_SCENES[0]


def scene_reference(scene, thr, lq):
    """(gt_inds int64 [B,Nmax] with -1 at and beyond nbox, [max_ov float32 [nbox_b]] per image)."""
    B, nmax = scene['boxes'].shape[:2]
    gi = np.full((B, nmax), -1, np.int64)
    mo = []
    for b in range(B):
        nb, ng = int(scene['nbox'][b]), int(scene['ngt'][b])
        g, m = assign_reference(scene['boxes'][b, :nb], scene['gts'][b, :ng], thr[0], thr[1], thr[2], lq)
        gi[b, :nb] = g
        mo.append(m)
    return gi, mo


def scene_census(scene):
    """Counts of the geometric situations in the live part of a scene (they do not depend on the thresholds)."""
    c = dict(shared_max=0, dup_gt=0, later_block_only=0, two_blocks=0, touching=0, empty_box=0, empty_gt=0, two_unmatched=0,
             ends_in_wave=0, no_gt=0)
    for b in range(scene['boxes'].shape[0]):
        nb, ng = int(scene['nbox'][b]), int(scene['ngt'][b])
        c['ends_in_wave'] += int(nb % WAVE != 0 and nb < scene['boxes'].shape[1])
        c['no_gt'] += int(ng == 0)
        if nb == 0 or ng == 0:
            continue
        boxes, gts = scene['boxes'][b, :nb], scene['gts'][b, :ng]
        ov = iou_matrix(gts, boxes)
        gm = ov.max(1)
        hit = (ov == gm[:, None]) & (gm[:, None] > 0)
        c['shared_max'] += int((hit.sum(1) > 1).sum())
        c['dup_gt'] += int(np.triu((gts[:, None, :] == gts[None, :, :]).all(-1), 1).sum())
        blocks = np.zeros((ng, -(-nb // BLOCK)), bool)
        gi, bi = np.nonzero(hit)
        blocks[gi, bi // BLOCK] = True
        c['later_block_only'] += int((blocks.any(1) & ~blocks[:, 0]).sum())
        c['two_blocks'] += int((blocks.sum(1) > 1).sum())
        g, x = gts[:, None, :], boxes[None, :, :]
        edge = ((g[..., 2] == x[..., 0]) | (g[..., 0] == x[..., 2])) & (np.minimum(g[..., 3], x[..., 3]) > np.maximum(g[..., 1], x[..., 1]))
        c['touching'] += int((edge & (ov == 0)).sum())
        c['empty_box'] += int(((boxes[:, 2] == boxes[:, 0]) | (boxes[:, 3] == boxes[:, 1])).sum())
        c['empty_gt'] += int(((gts[:, 2] == gts[:, 0]) | (gts[:, 3] == gts[:, 1])).sum())
        c['two_unmatched'] += int((gm == 0).sum() >= 2)
    return c


def threshold_census(scene, thr):
    """How many box maxima lie on / below / above pos_thr and neg_thr, and how many gt maxima on / below / above min_pos."""
    c = dict(pos_eq=0, pos_below=0, pos_above=0, neg_eq=0, neg_below=0, neg_above=0, min_eq=0, min_below=0, min_above=0)
    for b in range(scene['boxes'].shape[0]):
        nb, ng = int(scene['nbox'][b]), int(scene['ngt'][b])
        if nb == 0 or ng == 0:
            continue
        ov = iou_matrix(scene['gts'][b, :ng], scene['boxes'][b, :nb])
        for name, v, t in (('pos', ov.max(0), F32(thr[0])), ('neg', ov.max(0), F32(thr[1])), ('min', ov.max(1), F32(thr[2]))):
            c[name + '_eq'] += int((v == t).sum())
            c[name + '_below'] += int((v < t).sum())
            c[name + '_above'] += int((v > t).sum())
    return c
