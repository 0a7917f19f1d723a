"""CPU: the loss launch (fused_loss_kernel), the narrow-head backward (narrow_head_bwd_kernel, both in csrc/elementwise.hip) and the RPN
normaliser (sampled_avg_factor_kernel, csrc/boxes.hip) without a GPU -- the float64 references, the case tables
tests/test_loss_forms_gpu.py runs, their censuses, the references against oracle/ops_ref.py, the recorded values of tests/golden/ and
torch.autograd, K._loss_view against brute-force offsets, and what the entry points refuse.

References are float64 numpy over operands already rounded to their types; torch appears only where a value is rounded to a type or an
oracle is called.  reference_loss follows the comment block above fused_loss_kernel and loft/losses.py:
    loss = k sum_i w_i l_i,   grad_i = k w_i dl_i/dp_i,   k = scale / denom
    L1 l = |d|;  SmoothL1 l = d^2 / (2 beta) if |d| < beta else |d| - beta / 2   (d = p - t);
    BCE l = max(p, 0) - p t + log1p(exp(-|p|)), dl/dp = sigmoid(p) - t;   CE l = mx + log(sum exp(p - mx)) - p[lab], softmax - onehot.
Next to every value it returns the same expression over the absolute values of its addends (`mag`): a rounding error of the fp32
evaluation is relative to that, not to the value, wherever addends cancel.

LOSS_FORMS: every mode (L1, SmoothL1 at beta 1, 1/2, 1/9, BCE on fp32 targets and on int64 labels, CE at C = 1, 2, 5 with and without
the accuracy count) meets every n, every pred addressing, every weight kind and every denominator kind at least once
(test_loss_census).  A row is launched through the entry point with NaN-filled outputs unless the wrapper is what it tests: a view
that does not collapse to three dims (the contiguous fallback) and an int64 denominator (the cast) exist only in K.fused_loss.
NH_FORMS: one row per instantiation of narrow_head_bwd_kernel, 20 in all (test_nh_census)."""
import functools
import itertools
import os
import zlib

import numpy as np
import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import lib as L

F = np.float32
U = 2.0 ** -24
E_ULP = 2          # expf / logf / log1pf / division: the installed ROCm ships no OCML accuracy table (no document or header under it
#                    states a maximum for these), so 2 ulp is assumed, twice the 1 ulp OpenCL full profile asks of exp and log1p
BIG = 262144 + 1025
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- references ---------------------------------------------------------------------------------------------------------------------
def reference_loss(mode, pred, target, weight, denom, scale, beta=1.0):
    """mode 'l1' | 'smooth_l1' | 'bce' | 'ce'; pred fp32 [n] ([n, C] for 'ce'); target fp32 [n], or int64 [n] (labels: 'bce' takes
    label >= 1, 'ce' the class); weight None or one value per element (row for 'ce'), bool or fp32; denom, scale, beta fp32 values.
    -> dict: k, w; l, mag (per element, unweighted); grad, gmag (per element, weighted by k w); total = k sum w l,
    mag_total = |k| sum |w l|, mag_terms = |k| sum |w| mag; for 'ce' hits (first maximum on ties) and the pieces of the gradient's
    conditioning (soft = |k w| softmax, lse_abs = |mx| + |log se|, arg_abs = |p - lse|)."""
    p = np.asarray(pred, np.float64)
    k = float(F(scale)) / float(F(denom))
    n = p.shape[0]
    w = np.ones(n) if weight is None else np.asarray(weight).astype(np.float64)
    out = dict(k=k, w=w)
    if mode == 'ce':
        lab = np.asarray(target).astype(np.int64)
        C = p.shape[1]
        mx = p.max(1)
        se = np.exp(p - mx[:, None]).sum(1)
        lse = mx + np.log(se)
        rows = np.arange(n)
        l = lse - p[rows, lab]
        mag = np.abs(mx) + np.abs(np.log(se)) + np.abs(p[rows, lab])
        soft = np.exp(p - lse[:, None])
        hot = np.zeros((n, C))
        hot[rows, lab] = 1.0
        kw = (k * w)[:, None]
        out.update(grad=kw * (soft - hot), gmag=np.abs(kw) * (soft + hot), soft=np.abs(kw) * soft,
                   lse_abs=(np.abs(mx) + np.abs(np.log(se)))[:, None] * np.ones((1, C)), arg_abs=np.abs(p - lse[:, None]),
                   hits=int((np.argmax(p, 1) == lab).sum()))
    else:
        t = np.asarray(target)
        t = (t >= 1).astype(np.float64) if t.dtype.kind in 'iu' else t.astype(np.float64)
        if mode == 'bce':
            soft = np.log1p(np.exp(-np.abs(p)))
            l = np.maximum(p, 0) - p * t + soft
            mag = np.maximum(p, 0) + np.abs(p * t) + soft
            e = np.exp(-np.abs(p))
            sig = np.where(p >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            g, gm = sig - t, sig + np.abs(t)
        else:
            b = float(F(beta))
            d = p - t
            ad = np.abs(d)
            if mode == 'l1':
                l, mag, g = ad, ad, np.sign(d)
            else:
                quad = ad < b
                l = np.where(quad, 0.5 * d * d / b, ad - 0.5 * b)
                mag = np.where(quad, l, ad + 0.5 * b)
                g = np.where(quad, d / b, np.sign(d))
            gm = np.abs(g)
        out.update(grad=k * w * g, gmag=np.abs(k * w) * gm)
    out.update(l=l, mag=mag, total=k * float((w * l).sum()), mag_total=abs(k) * float(np.abs(w * l).sum()),
               mag_terms=abs(k) * float((np.abs(w) * mag).sum()))
    return out


def reference_narrow_bwd(g, x, w, relu_in):
    """g [M, Cout], x [M, Cin], w [Cout, Cin] -> gx = [x > 0] (g w), dw = g^T x, db = colsum g and their sums of absolute terms."""
    g, x, w = (np.asarray(a, np.float64) for a in (g, x, w))
    keep = (x > 0) if relu_in else np.ones(x.shape, bool)
    return dict(gx=np.where(keep, g @ w, 0.0), dw=g.T @ x, db=g.sum(0),
                mag_gx=np.where(keep, np.abs(g) @ np.abs(w), 0.0), mag_dw=np.abs(g).T @ np.abs(x), mag_db=np.abs(g).sum(0))


def reference_avg_factor(pv, nv):
    """sum_b max(#pos_b, 1) + sum_b max(#neg_b, 1) over validity bytes [B, P] / [B, Q] (any non-zero byte is valid)."""
    return sum(max(int(np.count_nonzero(r)), 1) for r in pv) + sum(max(int(np.count_nonzero(r)), 1) for r in nv)


# ---- the loss table -------------------------------------------------------------------------------------------------------------------
MODES = {
    'l1': dict(code=0, kernel='l1', C=0, beta=1.0), 'sl1_1': dict(code=1, kernel='smooth_l1', C=0, beta=1.0),
    'sl1_half': dict(code=1, kernel='smooth_l1', C=0, beta=0.5), 'sl1_ninth': dict(code=1, kernel='smooth_l1', C=0, beta=1.0 / 9.0),
    'bce': dict(code=2, kernel='bce', C=0, beta=1.0), 'bce_lab': dict(code=2, kernel='bce', C=0, beta=1.0, labels=True),
}
for _c in (1, 2, 5):
    MODES[f'ce{_c}'] = dict(code=3, kernel='ce', C=_c, beta=1.0)
    MODES[f'ce{_c}_acc'] = dict(code=3, kernel='ce', C=_c, beta=1.0, acc=True)
NS = (1, 255, 1024, 1025, BIG)
VIEWS = ('dense', 'cols', 'rows_bs5', 'nhwc', 'noncollapse')
WEIGHTS = ('none', 'f32', 'bool', 'bool_row', 'zero')
DENOMS = ('dev_f32', 'dev_i64', 'number', 'none')
EXACT_MODES = ('l1', 'sl1_1', 'sl1_half')
_FACTOR4 = {1024: (4, 4, 8, 8), BIG: (27, 27, 19, 19)}


def view_of(kind, n, C):
    """-> (shape of the wider buffer, f(buffer) = the logical pred view, row_dims).  Elementwise modes (C == 0): the view has n
    elements; 'ce': n rows of C classes at unit stride ('noncollapse': a transposed [C, n], which the wrapper must make contiguous)."""
    if C == 0:
        if kind == 'dense':
            return (n,), (lambda b: b), 1
        if kind == 'cols':                                   # columns [2 : 2 + w] of an [n / w, 8] head output
            wd = next(d for d in (4, 5, 3, 1) if n % d == 0)
            return (n // wd, 8), (lambda b: b[:, 2:2 + wd]), 2
        if kind == 'rows_bs5':                               # rows b, p < P, columns 1..4 of the RPN's [B, S, 5] gather
            bp = n // 4
            nb = 2 if bp % 2 == 0 else 1
            return (nb, bp // nb + 3, 5), (lambda b: b[:, :bp // nb, 1:5]), 3
        if kind == 'nhwc':                                   # one channel of a 4-padded NHWC map
            return (1, 1, n, 4), (lambda b: b[..., 2]), 3
        a, b_, c, d = _FACTOR4[n]
        return (a, b_ + 1, c + 1, d + 1), (lambda b: b[:, :b_, :c, :d]), 4
    if kind == 'dense':
        return (n, C), (lambda b: b), 1
    if kind == 'cols':
        return (n, 8), (lambda b: b[:, 1:1 + C]), 1
    if kind == 'rows_bs5':
        nb = next((d for d in (2, 3, 5) if n % d == 0), 1)
        return (nb, n // nb + 3, 8), (lambda b: b[:, :n // nb, 2:2 + C]), 2
    if kind == 'nhwc':
        return (1, 1, n, 8), (lambda b: b[0, 0, :, :C]), 1
    return (C, n), (lambda b: b.t()), 1


def _wrapper_row(view, denom):
    return view == 'noncollapse' or denom == 'dev_i64'


def _compatible(mode, n, view, weight, denom):
    C = MODES[mode]['C']
    if not _wrapper_row(view, denom):
        return True
    if C and view == 'rows_bs5':                             # a [B, P, C] view is no 2-D pred
        return False
    if weight == 'bool_row':                                 # the wrapper spells it as a weight expanded over the last dim
        return C == 0 and view in ('cols', 'rows_bs5', 'noncollapse') and not (view == 'cols' and n == 1)
    return True


def _build_loss_forms():
    rows = []
    for mi, mode in enumerate(MODES):
        C = MODES[mode]['C']
        if C == 0:
            free = [('dense', 'cols', 'nhwc')[(j + mi) % 3] for j in range(3)]
            pairs = [(1, free[0]), (255, free[1]), (1024, 'rows_bs5'), (1025, free[2]), (BIG, 'noncollapse'), (BIG, 'dense')]
        else:
            pairs = [(NS[j], VIEWS[(j + mi) % 5]) for j in range(5)]
            pairs.append((BIG, 'cols' if (BIG, 'dense') in pairs else 'dense'))
        rot = lambda s, r: tuple(s[(i + r) % len(s)] for i in range(len(s)))
        cand_w = [rot(WEIGHTS, mi + r) for r in range(5)] + list(itertools.permutations(WEIGHTS))
        cand_d = [rot(DENOMS, mi + r) for r in range(4)]
        pick = next((ws, ds) for ws in cand_w for ds in cand_d
                    if all(_compatible(mode, n, v, ws[j], ds[j % 4]) for j, (n, v) in enumerate(pairs[:5])))
        ws, ds = pick[0] + ('f32',), tuple(pick[1][j % 4] for j in range(5)) + ('dev_f32',)
        for j, (n, v) in enumerate(pairs):
            rows.append(dict(id=f'{mode}-{n}-{v}-{ws[j]}-{ds[j]}', mode=mode, n=n, view=v, weight=ws[j], denom=ds[j],
                             via='wrapper' if _wrapper_row(v, ds[j]) else 'entry'))
    return rows


LOSS_FORMS = _build_loss_forms()
LOSS_IDS = [r['id'] for r in LOSS_FORMS]

EDGE_LOGITS = [0.0] + [s * v for v in (2.0 ** -20, 20.0, 88.0, 104.0) for s in (1.0, -1.0)]


def _edge_block(mode):
    """-> (pred rows, targets, unit-or-zero weights): every edge logit, ties, the [100, -100] row, every label value, each once with
    weight 1 and once with weight 0."""
    C = MODES[mode]['C']
    if C == 0:
        labs = (0, 1, 2) if MODES[mode].get('labels') else (0.0, 1.0, 0.25)
        cells = [(v, t) for v in EDGE_LOGITS for t in labs]
    else:
        base = [[v] + [0.0] * (C - 1) for v in EDGE_LOGITS] + [[v] * C for v in EDGE_LOGITS]
        if C >= 2:
            base += [[100.0, -100.0] + [0.0] * (C - 2), [-100.0, 100.0] + [0.0] * (C - 2), [0.0, -20.0] + [-20.0] * (C - 2),
                     [1.0] * 2 + [0.0] * (C - 2), [0.0] * (C - 2) + [1.0] * 2]
        cells = [(r, t) for r in base for t in range(C)]
    cells = [(p, t, wv) for wv in (1.0, 0.0) for p, t in cells]
    return ([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])


def _is_pow2(v):
    return v > 0 and float(np.log2(v)).is_integer()


def loss_operands(row, exact=False):
    """The operands of a LOSS_FORMS row, rounded to their types.  exact: class (A), L1 / SmoothL1 on the dyadic lattice (multiples
    of 1/8 up to 4; of 1/2 up to 1 at the large n, so that the partial sums stay below 2^24 grains), power-of-two scale and
    denominator, with d == 0 and |d| == beta among the elements.  Otherwise class (B): random, behind the fixed edge block for
    BCE / CE.  -> dict(pred, target, weight (per stored weight, None | fp32 | uint8), wdiv, w_elem (per element / row), denom_kind,
    denom, scale, beta)."""
    m = MODES[row['mode']]
    n, C = row['n'], m['C']
    rng = np.random.default_rng(zlib.crc32((row['id'] + ('A' if exact else 'B')).encode()))
    beta = float(F(m['beta']))
    if exact:
        assert row['mode'] in EXACT_MODES
        step, top = (0.5, 1.0) if n > 4096 else (0.125, 4.0)
        q = int(top / step)
        pred = (rng.integers(-q, q + 1, n) * step).astype(F)
        target = (rng.integers(-q, q + 1, n) * step).astype(F)
        for i, d in enumerate((0.0, beta, -beta)[:n]):       # d == 0, |d| == beta
            target[i] = pred[i] - F(d)
    elif C == 0:
        pred = rng.normal(0, 3, n).astype(F)
        if m['kernel'] == 'bce':
            target = rng.integers(0, 3, n) if m.get('labels') else np.where(rng.random(n) < 0.5, rng.integers(0, 2, n), rng.random(n)).astype(F)
        else:                                                # both branches of SmoothL1 at every beta
            target = (pred + rng.normal(0, 1, n) * rng.choice([0.05, 1.0], n)).astype(F)
    else:
        pred = rng.normal(0, 3, (n, C)).astype(F)
        target = rng.integers(0, C, n)
    wk = row['weight']
    wide = row['via'] == 'wrapper' and wk == 'bool_row'
    wdiv = (view_of(row['view'], n, C)[1](torch.empty(view_of(row['view'], n, C)[0])).shape[-1] if wide else 4) if wk == 'bool_row' else 1
    nw = (n + wdiv - 1) // wdiv
    if wk == 'none':
        weight = None
    elif wk == 'f32':
        weight = rng.choice(np.array([0.25, 3.0, 1.0, 0.0, 0.5] if exact else [0.25, 3.0, 1.0, 0.0, 0.7], F), nw)
    elif wk == 'zero':
        weight = np.zeros(nw, F) if zlib.crc32(row['id'].encode()) % 2 else np.zeros(nw, np.uint8)
    else:
        weight = (rng.random(nw) < 0.7).astype(np.uint8)
    if not exact and m['kernel'] in ('bce', 'ce'):           # the edge block, in front
        ep, et, ew = _edge_block(row['mode'])
        idx = np.arange(len(ep)) if n >= len(ep) else np.sort(rng.choice(len(ep), n, replace=False))
        pred[:len(idx)] = np.asarray(ep, F)[idx]
        target[:len(idx)] = np.asarray(et)[idx].astype(target.dtype)
        if wk in ('f32', 'bool'):
            weight[:len(idx)] = np.asarray(ew)[idx].astype(weight.dtype)
    w_elem = None if weight is None else np.repeat(weight, wdiv)[:n]
    dk = row['denom']
    if exact:
        if dk == 'none' and not _is_pow2(n):
            dk = 'number'                                    # count = n is no power of two: a python number in its place
        denom = {'dev_f32': 4.0, 'dev_i64': 8.0, 'number': 32.0, 'none': float(n)}[dk]
        scale = 2.0
    else:
        denom = {'dev_f32': 37.5, 'dev_i64': 41.0, 'number': float(F(0.75 * n + 1.0)), 'none': float(n)}[dk]
        scale = float(F(1.7))
    return dict(pred=pred, target=target, weight=weight, wdiv=wdiv, w_elem=w_elem, denom_kind=dk, denom=denom, scale=scale, beta=beta)


@functools.lru_cache(maxsize=4)
def loss_problem(rid, exact=False):
    """(operands, reference) of the row with id `rid`, computed once and shared."""
    row = LOSS_FORMS[LOSS_IDS.index(rid)]
    op = loss_operands(row, exact)
    ref = reference_loss(MODES[row['mode']]['kernel'], op['pred'], op['target'], op['w_elem'], op['denom'], op['scale'], op['beta'])
    for a in list(op.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return op, ref


def launch_blocks(n):
    return 1 if n <= 0 else min((n + 1023) // 1024, 256)


def sum_depth(n):
    """Roundings between one term and loss_out[0], read from fused_loss_kernel: the thread's serial additions, 6 shuffle steps,
    3 additions of wave partials, one addition per block in the last block's loop."""
    b = launch_blocks(n)
    return -(-n // (b * 256)) + 6 + 3 + b


def _pow2_grain(a):
    """The largest power of two (<= 1) of which every entry of `a` is an integer multiple."""
    g = 1.0
    while not np.array_equal(a / g, np.round(a / g)):
        g /= 2
        assert g >= 2.0 ** -20, 'not on a dyadic lattice'
    return g


def loss_grain_ok(ref):
    """Every term w_i l_i is an integer multiple of g and sum |w_i l_i| < 2^24 g: every partial sum, in any order and grouping, is
    exact in fp32; k is a power of two."""
    terms = ref['w'] * ref['l']
    g = _pow2_grain(terms)
    return _is_pow2(abs(ref['k'])) and float(np.abs(terms).sum()) / g < 2 ** 24


def test_loss_census():
    seen = {m: dict(n=set(), view=set(), weight=set(), denom=set()) for m in MODES}
    for r in LOSS_FORMS:
        for ax in ('n', 'view', 'weight', 'denom'):
            seen[r['mode']][ax].add(r[ax])
        assert _compatible(r['mode'], r['n'], r['view'], r['weight'], r['denom']), r['id']
    for m, s in seen.items():
        assert s['n'] == set(NS) and s['view'] == set(VIEWS) and s['weight'] == set(WEIGHTS) and s['denom'] == set(DENOMS), (m, s)
    assert len(set(LOSS_IDS)) == len(LOSS_IDS) == 6 * len(MODES)
    assert {MODES[m]['C'] for m in MODES} == {0, 1, 2, 5} and {float(F(MODES[m]['beta'])) for m in MODES} == {1.0, 0.5, float(F(1 / 9))}
    # the large n runs capped: every thread strides more than four times, the accuracy partials reach partial[256 + 255]
    assert launch_blocks(BIG) == 256 and -(-BIG // (256 * 256)) > 4 and launch_blocks(262144) == 256 and launch_blocks(1025) == 2
    assert any(r['via'] == 'entry' and r['n'] == BIG and MODES[r['mode']].get('acc') for r in LOSS_FORMS)


@pytest.mark.parametrize('rid', [r['id'] for r in LOSS_FORMS if r['n'] <= 1025])
def test_loss_operands_hold_what_the_table_promises(rid):
    row = LOSS_FORMS[LOSS_IDS.index(rid)]
    op, ref = loss_problem(rid)
    m = MODES[row['mode']]
    shape, f, _ = view_of(row['view'], row['n'], m['C'])
    v = f(torch.empty(shape))
    assert v.numel() == row['n'] * max(m['C'], 1)
    assert np.isfinite(ref['grad']).all() and np.isfinite(ref['total'])
    if m['kernel'] in ('bce', 'ce') and row['n'] >= 255:
        flat = set(np.abs(op['pred']).ravel().tolist())
        assert {2.0 ** -20, 20.0, 88.0, 104.0} <= flat
        assert set(np.asarray(op['target']).tolist()) >= ({0, 1, 2} if m.get('labels') else set(range(max(m['C'], 1))))
    if m['kernel'] == 'smooth_l1' and row['n'] >= 255:
        quad = np.abs(op['pred'].astype(np.float64) - op['target']) < op['beta']
        assert quad.any() and not quad.all()
    if row['weight'] == 'zero':
        assert ref['total'] == 0 and not ref['grad'].any()
    if row['mode'] in EXACT_MODES:
        opa, refa = loss_problem(rid, True)
        assert loss_grain_ok(refa), rid
        d = opa['pred'].astype(np.float64) - opa['target']
        assert d[0] == 0 and (row['n'] < 3 or (d[1] == opa['beta'] and d[2] == -opa['beta']))
        g32 = refa['grad'].astype(F).astype(np.float64)
        assert np.array_equal(g32, refa['grad']) and float(F(refa['total'])) == refa['total']


@pytest.mark.parametrize('rid', [r['id'] for r in LOSS_FORMS if r['n'] == BIG and r['mode'] in EXACT_MODES])
def test_large_exact_rows_stay_below_2_24_grains(rid):
    _, refa = loss_problem(rid, True)
    assert loss_grain_ok(refa)


# ---- the references against the oracle, the recorded values and autograd -------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.array(a))


def _oracle_loss(mode, pred, target, weight, denom, scale, beta):
    """oracle/ops_ref.py in float64 on the same operands; -> (loss, d loss / d pred) as numpy."""
    from oracle import ops_ref as R
    p = _t(np.asarray(pred, np.float64)).requires_grad_(True)
    n = p.shape[0]
    w = torch.ones(n, dtype=torch.float64) if weight is None else _t(np.asarray(weight, np.float64))
    if mode == 'ce':
        loss = R.ce_loss(p, _t(target), w, denom)
    elif mode == 'bce' and np.asarray(target).dtype.kind in 'iu':
        loss = R.bce_sigmoid_loss(p.view(-1, 1), _t(target), w, denom)
    elif mode == 'bce':                                      # fp32 targets: the mask form, one channel, plain mean over n
        assert weight is None and denom == n
        loss = R.mask_bce_loss(p.view(1, 1, n), _t(np.asarray(target, np.float64)).view(1, n), torch.zeros(1, dtype=torch.long))
    elif mode == 'l1':
        loss = R.l1_loss(p, _t(np.asarray(target, np.float64)), w, denom)
    else:
        loss = R.smooth_l1_loss(p, _t(np.asarray(target, np.float64)), beta=float(F(beta)), weight=w, avg_factor=denom)
    loss = loss.sum() * scale
    (g,) = torch.autograd.grad(loss, p)
    return float(loss.detach()), g.numpy()


ORACLE_ROWS = [r['id'] for r in LOSS_FORMS if r['n'] in (255, 1025) and r['view'] in ('dense', 'cols')]


@pytest.mark.parametrize('rid', ORACLE_ROWS)
def test_reference_loss_equals_the_oracle_in_float64(rid):
    """Value to 1e-12 relative to the sum of absolute addends; gradient to 1e-12 of its own sum of absolute addends (autograd of the
    ops_ref function in float64).  The weight-less fp32-target BCE goes through mask_bce_loss, the others through their own function.
    bce_sigmoid_loss casts its target to fp32 inside, which takes the whole torch expression to fp32: it is held to 2 * 2^-24 of the
    sum of absolute addends (its own precision), and the same labels go through mask_bce_loss in float64 at 1e-12 as well."""
    row = LOSS_FORMS[LOSS_IDS.index(rid)]
    op, ref = loss_problem(rid)
    mode = MODES[row['mode']]['kernel']
    w, denom = op['w_elem'], float(F(op['denom']))
    if mode == 'bce' and not MODES[row['mode']].get('labels'):
        w, denom = None, float(row['n'])
        ref = reference_loss(mode, op['pred'], op['target'], None, denom, op['scale'], op['beta'])
    want, grad = _oracle_loss(mode, op['pred'], op['target'], w, denom, float(F(op['scale'])), op['beta'])
    tol = 1e-12
    if MODES[row['mode']].get('labels'):
        tol = 4 * U
        hard = (np.asarray(op['target']) >= 1).astype(F)
        ref2 = reference_loss(mode, op['pred'], hard, None, float(row['n']), op['scale'], op['beta'])
        want2, grad2 = _oracle_loss(mode, op['pred'], hard, None, float(row['n']), float(F(op['scale'])), op['beta'])
        assert abs(ref2['total'] - want2) <= 1e-12 * ref2['mag_terms'] and (np.abs(ref2['grad'] - grad2) <= 1e-12 * ref2['gmag']).all()
    assert abs(ref['total'] - want) <= tol * max(ref['mag_terms'], 1e-300), (ref['total'], want)
    assert (np.abs(ref['grad'] - grad.reshape(ref['grad'].shape)) <= tol * ref['gmag'] + 1e-300).all()


def test_reference_loss_gives_the_recorded_values():
    """tests/golden/core_ops.npz l_*: the values tests/test_oracle_golden.py::test_losses pins the oracle to, at its tolerances, and the
    reference tree's two known answers exactly."""
    g = np.load(os.path.join(GOLD, 'core_ops.npz'))
    lg, lab, w = g['l_logits'], g['l_lab'], g['l_w']
    ce = reference_loss('ce', lg, lab, w, 37.0, 1.0)
    assert abs(ce['total'] - float(g['l_ce'])) < 1e-6
    assert abs(100.0 * ce['hits'] / len(lab) - float(g['l_acc'][0])) < 1e-4
    assert abs(reference_loss('bce', lg[:, 0], lab, w, 37.0, 1.0)['total'] - float(g['l_bce'])) < 1e-6
    a, b = g['l_a'].reshape(-1), g['l_b'].reshape(-1)
    assert abs(reference_loss('l1', a, b, np.repeat(w, 4), 50.0, 1.0)['total'] - float(g['l_l1'])) < 1e-5
    assert abs(reference_loss('smooth_l1', a, b, None, a.size, 16.0, 1.0)['total'] - float(g['l_sl1'])) < 1e-4
    mp, mt = g['l_mp'].reshape(-1), g['l_mt'].reshape(-1)
    assert abs(reference_loss('bce', mp, mt, None, mp.size, 1.0)['total'] - float(g['l_mask'][0])) < 1e-6
    fake = np.array([[100.0, -100.0]], F)
    assert reference_loss('ce', fake, np.array([1]), None, 1.0, 1.0)['total'] == 200.0
    assert reference_loss('ce', fake, np.array([0]), None, 1.0, 1.0)['total'] == 0.0
    tie = reference_loss('ce', np.zeros((4, 3), F), np.array([0, 1, 2, 0]), None, 1.0, 1.0)
    assert tie['hits'] == 2                                  # first maximum


def test_reference_narrow_bwd_equals_autograd_in_float64():
    rng = np.random.default_rng(5)
    g, x, w = rng.normal(size=(37, 3)), rng.normal(size=(37, 12)), rng.normal(size=(3, 12))
    x[::5] = 0.0
    for relu in (0, 1):
        xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
        bt = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        y = (torch.relu(xt) if relu else xt) @ wt.t() + bt
        gx, dw, db = torch.autograd.grad(y, (xt, wt, bt), _t(g))
        ref = reference_narrow_bwd(g, np.maximum(x, 0) if relu else x, w, relu)
        assert np.allclose(ref['gx'], gx.numpy(), rtol=1e-12, atol=1e-13)
        assert np.allclose(ref['dw'], dw.numpy(), rtol=1e-12, atol=1e-13) and np.allclose(ref['db'], db.numpy(), rtol=1e-12, atol=1e-13)
    assert reference_avg_factor(np.array([[0, 0], [1, 7]], np.uint8), np.zeros((2, 0), np.uint8)) == 1 + 2 + 1 + 1


# ---- K._loss_view --------------------------------------------------------------------------------------------------------------------
def view_offsets(view, n):
    """loss_view_off of csrc/elementwise.hip for logical indices 0..n-1."""
    d1, d2, s0, s1, s2 = view
    i = np.arange(n, dtype=np.int64)
    if d1 == 1 and d2 == 1:
        return i * s0
    i2, r = i % d2, i // d2
    return (r // d1) * s0 + (r % d1) * s1 + i2 * s2


def brute_offsets(t, row_dims):
    shape, stride = list(t.shape[:row_dims]), list(t.stride()[:row_dims])
    off = np.zeros(shape, np.int64)
    for ax, (n, st) in enumerate(zip(shape, stride)):
        sh = [1] * len(shape)
        sh[ax] = n
        off = off + (np.arange(n, dtype=np.int64) * st).reshape(sh)
    return off.reshape(-1)


def _sweep_views():
    base = torch.arange(2 * 7 * 6 * 10, dtype=torch.float32).view(2, 7, 6, 10)
    out = [('base', base), ('slice_last', base[..., 1:5]), ('slice_mid', base[:, :5, :, 3]), ('rows', base[:, :4, 2, 1:5]),
           ('step', base[:, ::2, :, ::3]), ('permuted', base.permute(3, 1, 0, 2)), ('permuted3', base[0].permute(2, 0, 1)),
           ('transposed', base[0, 0].t()), ('expanded', base[:, :, :1, :1].expand(2, 7, 6, 10)), ('expand_last', base[0, :, :, :1].expand(7, 6, 4)),
           ('size1', base[:1, :, :1, 4:5]), ('size1_mid', base[:, 2:3, :, 1:5]), ('one', base[1, 2, 3, 4:5]), ('scalar_rows', base[:1, :1, :1, :1]),
           ('four', base[:, :6, :5, :9]), ('four_step', base[:, ::3, ::2, ::4]), ('unsqueezed', base[0, 0, :, 2].unsqueeze(0).unsqueeze(-1)),
           ('all_expanded', base[:1, :1, :1, :1].expand(2, 7, 6, 10)), ('merge_two', base[:, :, :, :].reshape(14, 60)[:, :50])]
    for kind in VIEWS:
        for n in (1, 255, 1024, 1025):
            for C in (0, 2):
                if C == 0 and ((kind == 'rows_bs5' and n % 4) or (kind == 'noncollapse' and n not in _FACTOR4)):
                    continue
                shape, f, rd = view_of(kind, n, C)
                out.append((f'{kind}-{n}-{C}', f(torch.empty(shape))))
    return out


def test_loss_view_addresses_every_element_or_declines():
    declined = []
    for name, t in _sweep_views():
        for rd in range(1, t.dim() + 1):
            n = int(np.prod(t.shape[:rd]))
            v = K._loss_view(t, rd)
            if v is None:
                declined.append((name, rd))
                continue
            assert v[0] >= 1 and v[1] >= 1, (name, rd, v)
            assert np.array_equal(view_offsets(v, n), brute_offsets(t, rd)), (name, rd, v)
    # only views of four or more independent dims may be declined, and the table's 'noncollapse' view is one
    assert declined and all(name.startswith(('four', 'noncollapse', 'step', 'permuted')) for name, _ in declined), declined
    assert ('noncollapse-1024-0', 4) in declined
    for kind in ('dense', 'cols', 'rows_bs5', 'nhwc'):
        shape, f, rd = view_of(kind, 1024, 0)
        assert K._loss_view(f(torch.empty(shape)), f(torch.empty(shape)).dim()) is not None, kind


# ---- refusals: hipErrorInvalidValue (1), nothing launched ---------------------------------------------------------------------------
def _loss_code(mode=0, d1=1, d2=1, target_kind=0, weight_kind=0, wdiv=1, n=64, C=1, want_acc=0, partial=True, counter=True):
    """loft_fused_loss_v2's return code.  A refusal returns before anything is launched or dereferenced: without a device the buffers
    are made-up addresses; with one they are real and large enough, so a refusal that regressed fails the assert, not the machine."""
    if torch.cuda.is_available():
        keep = [torch.zeros(4096, device='cuda') for _ in range(5)] + [torch.zeros(4, dtype=torch.int32, device='cuda')]
        pp, tp, gp, pa, lo, cn = [t.data_ptr() for t in keep]
    else:
        pp = tp = gp = pa = lo = cn = 1 << 20
    code = L.load().loft_fused_loss_v2(mode, pp, d1, d2, max(C, 1), 0, 0, tp, target_kind, None, weight_kind, wdiv, n, C, None, 1.0, 1.0, 1.0,
                                       gp, pa if partial else None, cn if counter else None, lo, want_acc, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return code


LOSS_REFUSALS = [
    ('mode_-1', dict(mode=-1)), ('mode_4', dict(mode=4)), ('n_negative', dict(n=-1)), ('ce_without_classes', dict(mode=3, C=0)),
    ('no_partial', dict(partial=False)), ('no_counter', dict(counter=False)), ('d1_0', dict(d1=0)), ('d2_0', dict(d2=0)),
    ('wdiv_0', dict(wdiv=0)), ('target_kind_-1', dict(target_kind=-1)), ('target_kind_2', dict(target_kind=2)),
    ('labels_outside_bce_l1', dict(target_kind=1, mode=0)), ('labels_outside_bce_sl1', dict(target_kind=1, mode=1)),
    ('labels_outside_bce_ce', dict(target_kind=1, mode=3)), ('weight_kind_-1', dict(weight_kind=-1)), ('weight_kind_2', dict(weight_kind=2)),
    ('acc_l1', dict(want_acc=1, mode=0)), ('acc_sl1', dict(want_acc=1, mode=1)), ('acc_bce', dict(want_acc=1, mode=2)),
]


@pytest.mark.parametrize('case', LOSS_REFUSALS, ids=[c[0] for c in LOSS_REFUSALS])
def test_loss_refusals(case):
    assert _loss_code(**case[1]) == 1


def _nh_code(f32, Cin=16, Cout=2, g_stride=4, M=8):
    if torch.cuda.is_available():
        keep = [torch.zeros(M * 2048, device='cuda') for _ in range(6)]
        gp, xp, wp, gx, dw, db = [t.data_ptr() for t in keep]
    else:
        gp = xp = wp = gx = dw = db = 1 << 20
    fn = L.load().loft_narrow_head_bwd_f32 if f32 else L.load().loft_narrow_head_bwd
    code = fn(gp, g_stride, xp, wp, M, Cin, Cout, 0, gx, dw, db, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return code


NH_REFUSALS = [('cout_0', dict(Cout=0, g_stride=4)), ('cout_9', dict(Cout=9, g_stride=12)), ('cin_not_4n', dict(Cin=18)),
               ('cin_6', dict(Cin=6)), ('cin_1028', dict(Cin=1028)), ('g_stride_below_cout', dict(Cout=3, g_stride=2))]


@pytest.mark.parametrize('f32', (False, True), ids=('16bit', 'fp32'))
@pytest.mark.parametrize('case', NH_REFUSALS, ids=[c[0] for c in NH_REFUSALS])
def test_narrow_head_refusals(case, f32):
    assert _nh_code(f32, **case[1]) == 1


# ---- the narrow-head table ------------------------------------------------------------------------------------------------------------
NH_BIG_M = 32768 + 37


def nh_geometry(kind, Cout, Cin, M):
    """The launch geometry as loft_narrow_head_bwd / _f32 derive it: V, column groups, pixels per round, idle lanes, blocks, pixels
    per block, and the number of blocks whose range starts at or beyond M."""
    V = 8 if (kind == '16' and Cout <= 4 and Cin % 8 == 0) else 4
    cg = Cin // V
    ppi = max(256 // cg, 1)
    blocks = min(-(-M // (ppi * 16)), 2048) if M > 0 else 0
    per = -(-(-(-M // blocks)) // (ppi * 4)) * ppi * 4 if blocks else 0
    return dict(V=V, cg=cg, ppi=ppi, idle=256 - cg * ppi, blocks=blocks, per_blk=per,
                beyond=sum(1 for b in range(blocks) if b * per >= M), ragged=M % (ppi * 4) != 0)


def _nh_ms(kind, Cout, Cin):
    ppi = nh_geometry(kind, Cout, Cin, 1)['ppi']
    return (1, ppi * 4 - 1, ppi * 4 + 1, ppi * 16 * 3 + 5)


_NH_CIN = {('16', 8): (8, 256, 1024, 8), ('16', 4): (12, 1020, 12, 1020, 256, 1024, 12, 1020), ('32', 4): (8, 12, 256, 1020, 1024, 256, 12, 1020)}
NH_FORMS = ([dict(kind='16', Cout=c, Cin=_NH_CIN[('16', 8)][c - 1]) for c in range(1, 5)] +
            [dict(kind='16', Cout=c, Cin=_NH_CIN[('16', 4)][c - 1]) for c in range(1, 9)] +
            [dict(kind='32', Cout=c, Cin=_NH_CIN[('32', 4)][c - 1]) for c in range(1, 9)])
for _r in NH_FORMS:
    _r['Ms'] = _nh_ms(_r['kind'], _r['Cout'], _r['Cin'])
    _r['id'] = f"{_r['kind']}-cout{_r['Cout']}-cin{_r['Cin']}"
NH_IDS = [r['id'] for r in NH_FORMS]
NH_BIG = dict(kind='16', Cout=6, Cin=1024, id='16-cout6-cin1024-big')


def nh_dtype(kind):
    return torch.float32 if kind == '32' else L.act16()


def test_nh_census():
    inst = [(r['kind'], nh_geometry(r['kind'], r['Cout'], r['Cin'], 1)['V'], r['Cout']) for r in NH_FORMS]
    want = [('16', 8, c) for c in range(1, 5)] + [('16', 4, c) for c in range(1, 9)] + [('32', 4, c) for c in range(1, 9)]
    assert sorted(inst) == sorted(want) and len(set(inst)) == 20
    geo = {(r['Cin'], g['V']): g for r in NH_FORMS for g in [nh_geometry(r['kind'], r['Cout'], r['Cin'], 1)]}
    assert (geo[(8, 8)]['cg'], geo[(8, 8)]['ppi']) == (1, 256)
    assert (geo[(12, 4)]['cg'], geo[(12, 4)]['ppi'], geo[(12, 4)]['idle']) == (3, 85, 1)
    assert (256, 8) in geo and (256, 4) in geo
    assert (geo[(1020, 4)]['cg'], geo[(1020, 4)]['ppi'], geo[(1020, 4)]['idle']) == (255, 1, 1)
    assert geo[(1024, 8)]['ppi'] == 2 and geo[(1024, 4)]['ppi'] == 1
    for r in NH_FORMS:
        one, below, above, multi = (nh_geometry(r['kind'], r['Cout'], r['Cin'], M) for M in r['Ms'])
        assert r['Ms'][0] == 1 and one['blocks'] == 1
        assert below['ragged'] and above['ragged'] and r['Ms'][1] < one['ppi'] * 4 < r['Ms'][2]
        assert multi['blocks'] == 4 and multi['ragged'] and r['Ms'][3] % (one['ppi'] * 16)
    big = nh_geometry('16', 6, 1024, NH_BIG_M)
    # under the cap a block never starts beyond M (per_blk <= 16 ppi < M / (blocks - 1)); capped, per_blk's rounding leaves tail blocks idle
    assert big['V'] == 4 and big['blocks'] == 2048 and big['per_blk'] == 20 and big['beyond'] == 2048 - 1641
    assert all(nh_geometry(r['kind'], r['Cout'], r['Cin'], M)['beyond'] == 0 for r in NH_FORMS for M in r['Ms'])


def _round_to(a, dt):
    return a if dt == torch.float32 else torch.from_numpy(a).to(dt).float().numpy()


def nh_operands(kind, Cout, Cin, M, exact, seed=0):
    """g fp32 [M, c4] (channels Cout..c4-1 NaN, c4 > Cout), x [M, Cin] representable in the row's type with negatives, +0.0 and
    -0.0, w fp32 [Cout, Cin].  exact: integers of magnitude <= 4."""
    rng = np.random.default_rng(zlib.crc32(f'{kind}-{Cout}-{Cin}-{M}-{exact}-{seed}'.encode()))
    c4 = (Cout + 4) // 4 * 4
    g = np.full((M, c4), np.nan, F)
    if exact:
        g[:, :Cout] = rng.integers(-4, 5, (M, Cout))
        x = rng.integers(-4, 5, (M, Cin)).astype(F)
        w = rng.integers(-4, 5, (Cout, Cin)).astype(F)
    else:
        g[:, :Cout] = rng.normal(0, 1, (M, Cout))
        x = _round_to(rng.normal(0, 1, (M, Cin)).astype(F), nh_dtype(kind))
        w = rng.normal(0, 1, (Cout, Cin)).astype(F)
    z = rng.random((M, Cin))
    x[z < 0.05] = 0.0
    x[z > 0.95] = -0.0
    x.reshape(-1)[:3] = (-0.0 if seed % 2 else 0.0, -1.0, 0.0 if seed % 2 else -0.0)
    return g, x, w


@pytest.mark.parametrize('rid', NH_IDS)
def test_nh_exact_operands_are_exact_in_any_order(rid):
    r = NH_FORMS[NH_IDS.index(rid)]
    for M in r['Ms']:
        g, x, w = nh_operands(r['kind'], r['Cout'], r['Cin'], M, True)
        ref = reference_narrow_bwd(g[:, :r['Cout']], x, w, 1)
        assert max(ref['mag_gx'].max(), ref['mag_dw'].max(), ref['mag_db'].max()) < 2 ** 24
        assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all() and (x < 0).any() and (x > 0).any()
        assert np.isnan(g[:, r['Cout']:]).all() and g.shape[1] > r['Cout']
    assert NH_BIG_M * 16 < 2 ** 24 and 8 * 16 <= 256         # the large row's sums; |gx| <= 128 is exact in either 16-bit type


# ---- sampled_avg_factor ---------------------------------------------------------------------------------------------------------------
AVG_SHAPES = [(1, 1, 1), (1, 0, 300), (3, 257, 513), (6, 128, 256)]
AVG_FILLS = ('random', 'all_false', 'all_true', 'bytes')


def avg_operands(shape, fill):
    """uint8 [B, P], [B, Q]: 'bytes' holds values other than 1 (2, 128, 255) for valid; 'random' has one all-false and one all-true row."""
    B, P, Q = shape
    rng = np.random.default_rng(zlib.crc32(f'{shape}-{fill}'.encode()))
    if fill == 'all_false':
        return np.zeros((B, P), np.uint8), np.zeros((B, Q), np.uint8)
    if fill == 'all_true':
        return np.ones((B, P), np.uint8), np.ones((B, Q), np.uint8)
    pv, nv = (rng.random((B, P)) < 0.4).astype(np.uint8), (rng.random((B, Q)) < 0.6).astype(np.uint8)
    if fill == 'bytes':
        pv, nv = pv * rng.choice(np.array([2, 128, 255], np.uint8), (B, P)), nv * rng.choice(np.array([2, 128, 255], np.uint8), (B, Q))
    pv[0], nv[B - 1] = 0, 1
    return pv, nv


def test_avg_factor_reference():
    for shape in AVG_SHAPES:
        B, P, Q = shape
        assert reference_avg_factor(*avg_operands(shape, 'all_false')) == 2 * B
        assert reference_avg_factor(*avg_operands(shape, 'all_true')) == B * (max(P, 1) + max(Q, 1))
        pv, nv = avg_operands(shape, 'bytes')
        assert reference_avg_factor(pv, nv) == reference_avg_factor(pv != 0, nv != 0)
    assert max(avg_operands((3, 257, 513), 'bytes')[1].max(), 2) > 1
