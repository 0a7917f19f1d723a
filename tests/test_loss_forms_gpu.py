"""GPU: fused_loss_kernel, narrow_head_bwd_kernel (csrc/elementwise.hip) and sampled_avg_factor_kernel (csrc/boxes.hip) against the
float64 references of tests/test_loss_forms_cpu.py, row by row of its tables.

Losses.  A row goes through loft_fused_loss_v2 itself with caller-owned grad / loss_out / partial filled with NaN and everything of the
wider pred buffer outside the view NaN too ('entry'), or through K.fused_loss where the wrapper is what the row is about ('wrapper').
  (A) exact: L1 / SmoothL1(1, 1/2) on the dyadic lattice with power-of-two scale and denominator -- grad and loss EQUAL the reference
      (loss_grain_ok proves every partial sum exact); the branch boundary itself in test_smooth_l1_boundary.
  (B) bounded, u = 2^-24, E = E_ULP for every expf / logf / log1pf / division, counted from the kernel body:
      k = scale / denom: E.  grad_i = (k w) g: 2 roundings.
        L1       g = +-1.                                                    grad (2 + E) u |k w g|         -> c, t = 2, 1
        SmoothL1 d = p - t (1), g = d / beta (E).                             grad (3 + 2 E) u |k w g|       -> c, t = 3, 2
        BCE      g = 1 / (1 + expf(-p)) - t: expf E, 1 + e 1, 1 / x E, - t 1 on sigmoid + |t|.  grad (4 + 3 E) u |k w| (sig + |t|)
        CE       se = sum_c expf(p_c - mx): the arguments' roundings weigh |a| e^a <= 1/e each, the C - 1 additions 1 each, expf E:
                 se is good to (E + 2 C) u;  lse = mx + logf(se): E on |log se|, (E + 2 C) u absolute (log is ill-conditioned at
                 se ~ 1), 1 on |mx| + |log se|;  softmax s_c = expf(p_c - lse) carries the argument's absolute error as a relative
                 one:  s_c ((2 E + 2 C) + (E + 1)(|mx| + |log se|) + |p_c - lse|) u;  - onehot 1, k w 2, k E on s_c + onehot.
      l_i, relative to the sum of absolute addends mag_i:
        L1 d 1, w l 1 -> 2;   SmoothL1 d twice (d^2), d d 1, / beta E, w l 1 -> 4 + E;   BCE p t 1, -, + 2, w l 1, expf and log1pf
        E each (d log1p(x) / log1p(x) <= dx / x) -> 4 + 2 E;   CE lse 1, - p[lab] 1, w l 1, logf E -> 3 + E, plus (E + 2 C) u |w|.
      loss = k sum: sum_depth(n) roundings on sum |w l| (serial per thread, 6 shuffles, 3 wave partials, `blocks` in the last block),
      tot k 1, k E.  floor 2^-126 |k w| per term: whether fp32 subnormals survive is a compiler setting.
      No element is left out; the largest error / bound of each row is printed.  A test runs every row of its kernel family and
      names every row that missed (_every_row): the tables have some 130 rows, the suite one test per family.
  (C) accuracy = fp32 100 / n times the integer hits, first maximum on ties, written only with want_acc; partial[] entries written
      exactly for the launched blocks; the ticket counter back at 0; bit-identical repeats; autograd and the modules' fallbacks.
Narrow-head backward: (A) integers, dw / db / gx EQUAL in any order of the atomics; (B) gamma_NOUT u mag (+ one rounding to the 16-bit
type) for gx, (M + 1) u mag for dw (one product, at most M - 1 non-trivial additions on any path through registers, LDS and atomics:
adding an exact zero rounds nothing), M u mag for db; (C) need_* switches, M = 0."""

import numpy as np
import pytest
import torch

from test_loss_forms_cpu import (AVG_FILLS, AVG_SHAPES, BIG, E_ULP, EXACT_MODES, LOSS_FORMS, LOSS_IDS, MODES, NH_BIG, NH_BIG_M, NH_FORMS,
                                 NH_IDS, avg_operands, launch_blocks, loss_grain_ok, loss_problem, nh_dtype, nh_operands,
                                 reference_avg_factor, reference_loss, reference_narrow_bwd, sum_depth, view_of)

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
NAN = float('nan')
TINY = 2.0 ** -126


def _u16():
    from bonai_amd import lib as L
    return (2.0 ** -8, 0.0) if L.act16() == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- losses: launching a row --------------------------------------------------------------------------------------------------------
def _pred_view(row, op):
    m = MODES[row['mode']]
    shape, f, _ = view_of(row['view'], row['n'], m['C'])
    buf = torch.full(shape, NAN, device='cuda')
    view = f(buf)
    view.copy_(_dev(op['pred']).reshape(view.shape))
    return buf, view


def _run_entry(row, op, want_acc=None, counter=None):
    """loft_fused_loss_v2 on NaN-filled outputs -> dict(loss [2], grad, partial [512], counter), as numpy."""
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    m = MODES[row['mode']]
    n, C = row['n'], m['C']
    buf, view = _pred_view(row, op)
    vt = K._loss_view(view, view.dim() - (1 if C else 0))
    assert vt is not None
    target = _dev(op['target'])
    weight = None if op['weight'] is None else _dev(op['weight'])
    wkind = 0 if weight is None or weight.dtype == torch.float32 else 1
    af, count = None, NAN
    if op['denom_kind'] == 'dev_f32':
        af = torch.tensor([op['denom']], dtype=torch.float32, device='cuda')    # count must then go unread: NaN
    else:
        count = float(op['denom'])
    grad = torch.full((n * max(C, 1),), NAN, device='cuda')
    partial = torch.full((512,), NAN, device='cuda')
    out = torch.full((2,), NAN, device='cuda')
    counter = torch.zeros(1, dtype=torch.int32, device='cuda') if counter is None else counter
    acc = bool(m.get('acc')) if want_acc is None else want_acc
    L.check(L.load().loft_fused_loss_v2(m['code'], L.ptr(view), *vt, L.ptr(target), 1 if m.get('labels') else 0, L.ptr(weight), wkind,
                                        op['wdiv'], n, max(C, 1), L.ptr(af), count, op['scale'], op['beta'], L.ptr(grad), L.ptr(partial),
                                        L.ptr(counter), L.ptr(out), 1 if acc else 0, L.stream()), 'loft_fused_loss_v2')
    torch.cuda.synchronize()
    return dict(loss=out.double().cpu().numpy(), grad=grad.double().cpu().numpy(), partial=partial.double().cpu().numpy(),
                counter=int(counter.item()), acc=acc)


def _wrapper_args(row, op):
    m = MODES[row['mode']]
    buf, view = _pred_view(row, op)
    wk, weight = row['weight'], None
    if op['weight'] is not None:
        wt = _dev(op['weight'])
        wt = wt.bool() if wt.dtype == torch.uint8 else wt
        if wk == 'bool_row':
            weight = wt.reshape(view.shape[:-1] + (1,)).expand(view.shape)
        else:
            weight = wt if m['C'] else wt.reshape(view.shape)
    dk = op['denom_kind']
    af = {'dev_f32': lambda: torch.tensor(op['denom'], dtype=torch.float32, device='cuda'),
          'dev_i64': lambda: torch.tensor(int(op['denom']), dtype=torch.int64, device='cuda'),
          'number': lambda: float(op['denom']), 'none': lambda: None}[dk]()
    return view, _dev(op['target']), weight, af


def _run_wrapper(row, op):
    from bonai_amd import kernels as K
    m = MODES[row['mode']]
    view, target, weight, af = _wrapper_args(row, op)
    acc = bool(m.get('acc'))
    res = K.fused_loss(m['kernel'], view, target, weight, af, None, op['scale'], op['beta'], want_acc=acc,
                       target_ge1=bool(m.get('labels')))
    torch.cuda.synchronize()
    assert res[1].dtype == torch.float32 and tuple(res[1].shape) == tuple(view.shape)
    loss = np.array([float(res[0]), float(res[2]) if acc else NAN])
    return dict(loss=loss, grad=res[1].double().cpu().numpy().reshape(-1), partial=None, acc=acc,
                counter=int(next(iter(K._LOSS_SCRATCH.values())).item()))


def _run(row, op):
    return _run_entry(row, op) if row['via'] == 'entry' else _run_wrapper(row, op)


def loss_bounds(row, ref):
    """-> (per-element bound of grad, flattened; bound of loss_out[0]); the derivation is in the module docstring."""
    E, kern, C, n = E_ULP, MODES[row['mode']]['kernel'], MODES[row['mode']]['C'], row['n']
    kw = np.abs(ref['k'] * ref['w'])
    extra = 0.0
    if kern == 'ce':
        gb = U * (ref['soft'] * ((2 * E + 2 * C) + (E + 1) * ref['lse_abs'] + ref['arg_abs']) + (3 + E) * ref['gmag']) + TINY * kw[:, None]
        cl, tl = 3, 1
        extra = (E + 2 * C) * U * abs(ref['k']) * float(np.abs(ref['w']).sum())
    else:
        cg, tg = {'l1': (2, 1), 'smooth_l1': (3, 2), 'bce': (4, 3)}[kern]
        cl, tl = {'l1': (2, 0), 'smooth_l1': (4, 1), 'bce': (4, 2)}[kern]
        gb = (cg + E * tg) * U * ref['gmag'] + TINY * kw
    tb = (cl + E * tl) * U * ref['mag_terms'] + extra + (sum_depth(n) + 1 + E) * U * ref['mag_total'] + TINY * float(kw.sum())
    return gb.reshape(-1), tb


def expected_accuracy(hits, n):
    return float(F(hits) * (F(100.0) / F(n)))


def _check_outputs(row, got, ref):
    """What a launch owns: partial[b] and, with want_acc, partial[256 + b] for its blocks and nothing else; loss_out[1] only with
    want_acc; the ticket counter back at 0."""
    assert got['counter'] == 0
    if got['acc']:
        assert got['loss'][1] == expected_accuracy(ref['hits'], row['n']), (got['loss'][1], ref['hits'])
    else:
        assert np.isnan(got['loss'][1])
    if got['partial'] is not None:
        b = launch_blocks(row['n'])
        wrote = ~np.isnan(got['partial'])
        want = np.zeros(512, bool)
        want[:b] = True
        if got['acc']:
            want[256:256 + b] = True
            assert got['partial'][256:256 + b].sum() == ref['hits']
        assert np.array_equal(wrote, want), np.argwhere(wrote != want)[:4].tolist()


def _every_row(ids, check):
    """Run `check` on every row of a table and fail with ALL rows that missed, each named: one test per kernel family keeps the
    suite's test count small, and a failing row must not hide the rows behind it."""
    missed = []
    for rid in ids:
        try:
            check(rid)
        except AssertionError as e:
            missed.append(f'{rid}: {str(e)[:300]}')
    assert not missed, f'{len(missed)} of {len(ids)} rows:\n' + '\n'.join(missed)


KERNELS = ('l1', 'smooth_l1', 'bce', 'ce')


@pytest.mark.parametrize('kernel', KERNELS)
def test_loss_bounded(kernel):
    _every_row([r['id'] for r in LOSS_FORMS if MODES[r['mode']]['kernel'] == kernel], _loss_bounded_row)


def _loss_bounded_row(rid):
    row = LOSS_FORMS[LOSS_IDS.index(rid)]
    op, ref = loss_problem(rid)
    got = _run(row, op)
    gb, tb = loss_bounds(row, ref)
    err = np.abs(got['grad'] - ref['grad'].reshape(-1))
    lerr = abs(got['loss'][0] - ref['total'])
    rg, rl = float(np.nanmax(err / np.maximum(gb, 1e-300))), lerr / max(tb, 1e-300)
    print(f'RATIO loss {row["mode"]} grad {rg:.3f} value {rl:.3f} ({rid})')
    assert (err <= gb).all(), (rg, np.argwhere(~(err <= gb))[:4].tolist())
    assert lerr <= tb, (got['loss'][0], ref['total'], rl)
    _check_outputs(row, got, ref)
    if row['weight'] == 'zero':
        assert got['loss'][0] == 0 and not got['grad'].any()


def test_loss_exact():
    _every_row([r['id'] for r in LOSS_FORMS if r['mode'] in EXACT_MODES], _loss_exact_row)


def _loss_exact_row(rid):
    row = LOSS_FORMS[LOSS_IDS.index(rid)]
    op, ref = loss_problem(rid, True)
    assert loss_grain_ok(ref)
    got = _run(row, op)
    want = ref['grad'].reshape(-1)
    assert np.array_equal(got['grad'], want), np.argwhere(got['grad'] != want)[:4].tolist()
    assert got['loss'][0] == ref['total'], (got['loss'][0], ref['total'])
    _check_outputs(row, got, ref)


def _one(mode, p, t, beta):
    """One element, unit weight, scale = count = 1 through the entry point -> (loss, grad) as float64."""
    row = dict(mode=mode, n=1, view='dense')
    op = dict(pred=np.array([p], F), target=np.array([t], F), weight=None, wdiv=1, denom_kind='number', denom=1.0, scale=1.0, beta=float(F(beta)))
    got = _run_entry(row, op)
    return got['loss'][0], got['grad'][0]


def test_smooth_l1_boundary():
    """|d| == beta belongs to the linear branch (smooth_l1_loss.py: `diff < beta` is the quadratic one): l = |d| - beta / 2 = beta / 2
    and g = +-1, both exact in fp32 for ANY beta -- the quadratic expression 0.5 d d / beta rounds twice and underflows for a small
    beta.  One step inside (nextafter towards 0) is quadratic, one step outside linear with l = fl(|d| - beta / 2): one rounding of
    an exact difference whether or not the compiler contracts it.  d == 0 gives 0 and 0."""
    for beta in (1.0, 0.5, float(F(1.0 / 9.0)), float(F(0.3)), 2.0 ** -80):
        b = F(beta)
        for sg in (1.0, -1.0):
            l, g = _one('sl1_1', sg * b, 0.0, b)
            assert (l, g) == (0.5 * float(b), sg), ('at', beta, sg, l, g)
            out = np.nextafter(b, F(np.inf))
            l, g = _one('sl1_1', sg * out, 0.0, b)
            assert (l, g) == (float(F(float(out) - 0.5 * float(b))), sg), ('outside', beta, sg, l, g)
            ins = np.nextafter(b, F(0))
            l, g = _one('sl1_1', sg * ins, 0.0, b)
            ref = reference_loss('smooth_l1', np.array([sg * ins], F), np.array([0.0], F), None, 1.0, 1.0, b)
            if beta in (1.0, 0.5):                           # a power of two: every operation of the quadratic branch but d d is exact
                assert g == ref['grad'][0] and l == float(F(ref['total'])), ('inside', beta, sg, l, g)
            elif beta > 1e-10:
                assert abs(g - ref['grad'][0]) <= (1 + E_ULP) * U and abs(l - ref['total']) <= (2 + E_ULP) * U * ref['total']
        assert _one('sl1_1', 0.75, 0.75, b) == (0.0, 0.0)
        assert _one('l1', -0.0, 0.0, b) == (0.0, 0.0)


def _dense_bce(n, seed):
    row = dict(id=f'ticket-{n}', mode='bce', n=n, view='dense', weight='f32', denom='dev_f32', via='entry')
    rng = np.random.default_rng(seed)
    op = dict(pred=rng.normal(0, 3, n).astype(F), target=rng.random(n).astype(F), weight=rng.choice(np.array([0.25, 3.0, 0.0], F), n),
              wdiv=1, denom_kind='dev_f32', denom=37.5, scale=float(F(1.7)), beta=1.0)
    op['w_elem'] = op['weight']
    return row, op, reference_loss('bce', op['pred'], op['target'], op['weight'], op['denom'], op['scale'])


def test_repeats_are_bit_identical_and_the_ticket_counter_returns_to_zero():
    """n = 1, the capped n and n = 1025 back to back on one stream through the wrapper (its per-stream counter, K._LOSS_SCRATCH): each
    gives its own result, twice the same bits, and the counter reads 0 after each."""
    from bonai_amd import kernels as K
    probs = [_dense_bce(n, 11 + n) for n in (1, BIG, 1025)]
    args = [(_dev(op['pred']), _dev(op['target']), _dev(op['weight']), torch.tensor(op['denom'], device='cuda')) for _, op, _ in probs]
    runs = []
    for rep in range(2):                                     # no synchronisation between the six launches
        runs.append([K.fused_loss('bce', a[0], a[1], a[2], a[3], None, probs[i][1]['scale']) for i, a in enumerate(args)])
    torch.cuda.synchronize()
    counter = next(iter(K._LOSS_SCRATCH.values()))
    assert len(K._LOSS_SCRATCH) >= 1 and int(counter.item()) == 0
    for i, (row, op, ref) in enumerate(probs):
        gb, tb = loss_bounds(row, ref)
        l0, g0 = runs[0][i]
        l1, g1 = runs[1][i]
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
        assert abs(float(l0) - ref['total']) <= tb and (np.abs(g0.double().cpu().numpy() - ref['grad']) <= gb).all()
    for i, a in enumerate(args):                             # and one at a time, the counter read after each
        K.fused_loss('bce', a[0], a[1], a[2], a[3], None, probs[i][1]['scale'])
        assert all(int(c.item()) == 0 for c in K._LOSS_SCRATCH.values())
    own = torch.zeros(1, dtype=torch.int32, device='cuda')   # the entry point on a caller's counter, three launches on the same one
    for row, op, ref in probs:
        got = _run_entry(row, op, counter=own)
        assert got['counter'] == 0 and abs(got['loss'][0] - ref['total']) <= loss_bounds(row, ref)[1]


def test_accuracy_counts_the_first_maximum():
    n, C = 1025, 5
    lab = np.arange(n) % C
    for name, pred in (('zeros', np.zeros((n, C), F)), ('last_two', np.tile(np.array([0, 0, 0, 1, 1], F), (n, 1))),
                       ('first_and_last', np.tile(np.array([2, 0, 0, 1, 2], F), (n, 1)))):
        row = dict(mode='ce5_acc', n=n, view='dense')
        op = dict(pred=pred, target=lab, weight=None, wdiv=1, denom_kind='number', denom=float(n), scale=1.0, beta=1.0)
        ref = reference_loss('ce', pred, lab, None, float(n), 1.0)
        first = int(np.argmax(pred[0]))
        assert ref['hits'] == int((lab == first).sum())
        got = _run_entry(row, op)
        assert got['loss'][1] == expected_accuracy(ref['hits'], n), name
        _check_outputs(row, got, ref)
        off = _run_entry(row, op, want_acc=False)            # the same launch without the count owns neither output
        assert np.isnan(off['loss'][1]) and np.isnan(off['partial'][256:]).all() and off['loss'][0] == got['loss'][0]


# ---- autograd and the modules ---------------------------------------------------------------------------------------------------------
def _module_cases():
    from bonai_amd.loft.losses import CrossEntropyLoss, L1Loss, SmoothL1Loss
    rng = np.random.default_rng(3)
    n = 1025
    p4, t4 = rng.normal(0, 2, (n, 4)).astype(F), rng.normal(0, 2, (n, 4)).astype(F)
    w4 = rng.choice(np.array([0.0, 1.0, 0.25], F), (n, 4))
    lab2, lab01 = rng.integers(0, 2, n), rng.integers(0, 3, n)
    wr = rng.choice(np.array([0.0, 1.0, 3.0], F), n)
    pm, tm = rng.normal(0, 3, (9, 1, 7, 7)).astype(F), (rng.random((9, 7, 7)) < 0.5).astype(F)
    return [
        ('l1', L1Loss(loss_weight=1.5), 'l1', p4, (t4, w4), dict(avg_factor=300.0), (p4.reshape(-1), t4.reshape(-1), w4.reshape(-1), 300.0, 1.5, 1.0)),
        ('smooth_l1', SmoothL1Loss(beta=1.0 / 9.0, loss_weight=2.0), 'smooth_l1', p4, (t4, w4), dict(avg_factor=300.0),
         (p4.reshape(-1), t4.reshape(-1), w4.reshape(-1), 300.0, 2.0, 1.0 / 9.0)),
        ('ce', CrossEntropyLoss(loss_weight=0.75), 'ce', p4[:, :2], (lab2, wr), dict(avg_factor=77.0), (p4[:, :2], lab2, wr, 77.0, 0.75, 1.0)),
        ('sigmoid', CrossEntropyLoss(use_sigmoid=True, loss_weight=1.25), 'bce', p4[:, :1], (lab01, wr), dict(avg_factor=77.0),
         (p4[:, 0], lab01, wr, 77.0, 1.25, 1.0)),
        ('mask', CrossEntropyLoss(use_mask=True, loss_weight=1.0), 'bce', pm, (tm, np.zeros(9, np.int64)), dict(),
         (pm.reshape(-1), tm.reshape(-1), None, float(pm.size), 1.0, 1.0)),
    ]


def _ref_of(kern, refargs, pred):
    p, t, w, denom, scale, beta = refargs
    return reference_loss(kern, pred.reshape(p.shape), t, w, denom, scale, beta)


@pytest.mark.parametrize('sixteen', (False, True), ids=('fp32', '16bit'))
def test_autograd_scales_the_stored_gradient(sixteen):
    """pred.grad after (loss * s).backward() is s * grad within the (B) bound plus the product's rounding; for a 16-bit pred that value
    rounded once to the type.  The loss is evaluated on the values the 16-bit pred holds."""
    from bonai_amd import lib as L
    s = float(F(1.7))
    u16, tiny = _u16()
    for name, mod, kern, pred, rest, kw, refargs in _module_cases():
        dt = L.act16() if sixteen else torch.float32
        pt = _dev(np.ascontiguousarray(pred)).to(dt).requires_grad_(True)
        held = pt.detach().float().cpu().numpy()
        ref = _ref_of(kern, refargs, held)
        row = dict(mode={'l1': 'l1', 'smooth_l1': 'sl1_ninth', 'ce': 'ce2', 'bce': 'bce'}[kern], n=ref['l'].shape[0])
        gb, tb = loss_bounds(row, ref)
        loss = mod(pt, *[_dev(a) for a in rest], **kw)
        (loss.sum() * s).backward()
        assert abs(float(loss.detach().sum()) - ref['total']) <= tb, name
        want = s * ref['grad'].reshape(-1)
        bound = abs(s) * gb + U * np.abs(want)
        if sixteen:
            bound = bound + u16 * (np.abs(want) + bound) + tiny
        assert pt.grad.dtype == dt and pt.grad.shape == pt.shape
        err = np.abs(pt.grad.double().cpu().numpy().reshape(-1) - want)
        print(f'RATIO autograd {name} {"16" if sixteen else "32"} {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))


def test_module_fallbacks_keep_the_elementwise_path(monkeypatch):
    """class_weight, a reduction other than 'mean', an empty pred and the mask loss with avg_factor do not launch the fused kernel
    (K.fused_loss raises here) and still give the reference value: torch's fp32 elementwise chain, held to the (B) element bound with
    any-order summation (n roundings) and one more rounding for the class weight."""
    from bonai_amd import kernels as K
    from bonai_amd.loft.losses import CrossEntropyLoss, L1Loss, SmoothL1Loss

    def refuse(*a, **k):
        raise RuntimeError('the fused launch was taken')
    monkeypatch.setattr(K, 'fused_loss', refuse)
    rng = np.random.default_rng(9)
    n = 255
    p2, lab, wr = rng.normal(0, 2, (n, 2)).astype(F), rng.integers(0, 2, n), rng.choice(np.array([0.0, 1.0, 3.0], F), n)
    p4, t4 = rng.normal(0, 2, (n, 4)).astype(F), rng.normal(0, 2, (n, 4)).astype(F)

    def check(name, value, ref, mode):
        gb, tb = loss_bounds(dict(mode=mode, n=n), ref)
        tb = tb + (ref['l'].shape[0] + 1) * U * ref['mag_total']
        assert abs(float(value) - ref['total']) <= tb, (name, float(value), ref['total'])

    cw = np.array([0.5, 2.0], F)
    got = CrossEntropyLoss(class_weight=[0.5, 2.0], loss_weight=1.0)(_dev(p2), _dev(lab), _dev(wr), avg_factor=50.0)
    check('class_weight', got, reference_loss('ce', p2, lab, wr * cw[lab], 50.0, 1.0), 'ce2')
    got = L1Loss(reduction='sum', loss_weight=2.0)(_dev(p4), _dev(t4))
    check('sum', got, reference_loss('l1', p4.reshape(-1), t4.reshape(-1), None, 1.0, 2.0), 'l1')
    got = SmoothL1Loss(beta=0.5, loss_weight=1.0)(_dev(p4), _dev(t4), reduction_override='none')
    ref = reference_loss('smooth_l1', p4.reshape(-1), t4.reshape(-1), None, 1.0, 1.0, 0.5)
    assert got.shape == (n, 4) and (np.abs(got.double().cpu().numpy().reshape(-1) - ref['l']) <= (4 + E_ULP) * U * ref['mag'] + TINY).all()
    got = L1Loss()(torch.zeros(0, 4, device='cuda'), torch.zeros(0, 4, device='cuda'), avg_factor=3.0)
    assert float(got) == 0.0
    pm, tm = rng.normal(0, 3, (5, 1, 7, 7)).astype(F), (rng.random((5, 7, 7)) < 0.5).astype(F)
    with pytest.raises(AssertionError):                      # the elementwise mask_cross_entropy asserts avg_factor is None
        CrossEntropyLoss(use_mask=True)(_dev(pm), _dev(tm), _dev(np.zeros(5, np.int64)), avg_factor=4.0)
    monkeypatch.undo()
    got = CrossEntropyLoss(use_mask=True)(_dev(pm), _dev(tm), _dev(np.zeros(5, np.int64)))
    ref = reference_loss('bce', pm.reshape(-1), tm.reshape(-1), None, float(pm.size), 1.0)
    assert got.shape == (1,) and abs(float(got) - ref['total']) <= loss_bounds(dict(mode='bce', n=pm.size), ref)[1]


# ---- narrow-head backward -------------------------------------------------------------------------------------------------------------
def _nh_tensors(kind, g, x):
    M, c4 = g.shape
    gt = _dev(g).view(1, M, 1, c4).permute(0, 3, 1, 2)
    xt = _dev(x, nh_dtype(kind)).view(1, M, 1, x.shape[1]).permute(0, 3, 1, 2)
    return gt, xt


def _nh_entry(kind, Cout, g, x, w, relu):
    """The entry point on a NaN-filled gx and the wrapper's own zeroed dw / db -> float64 numpy (gx [M, Cin], dw, db)."""
    from bonai_amd import kernels as K
    from bonai_amd import lib as L
    M, Cin = x.shape
    gt, xt = _nh_tensors(kind, g, x)
    wt = _dev(w)
    gx = torch.full((M, Cin), NAN, dtype=nh_dtype(kind), device='cuda')
    dw, db = K.pooled_zeros((Cout, Cin), 'cuda'), K.pooled_zeros((Cout,), 'cuda')
    fn = L.load().loft_narrow_head_bwd_f32 if kind == '32' else L.load().loft_narrow_head_bwd
    L.check(fn(L.ptr(gt), g.shape[1], L.ptr(xt), L.ptr(wt), M, Cin, Cout, relu, L.ptr(gx), L.ptr(dw), L.ptr(db), L.stream()), 'narrow')
    torch.cuda.synchronize()
    return gx.double().cpu().numpy(), dw.double().cpu().numpy(), db.double().cpu().numpy()


def _round16(ref, dt):
    t = torch.from_numpy(np.ascontiguousarray(ref))
    assert torch.equal(t.float().double(), t), 'double rounding'
    return t.float().to(dt).double().numpy()


def test_narrow_head_exact():
    _every_row(NH_IDS, _narrow_head_exact_row)


def _narrow_head_exact_row(rid):
    r = NH_FORMS[NH_IDS.index(rid)]
    for M in r['Ms']:
        for relu in (0, 1):
            g, x, w = nh_operands(r['kind'], r['Cout'], r['Cin'], M, True, relu)
            ref = reference_narrow_bwd(g[:, :r['Cout']], x, w, relu)
            assert max(ref['mag_gx'].max(), ref['mag_dw'].max(), ref['mag_db'].max()) < 2 ** 24
            gx, dw, db = _nh_entry(r['kind'], r['Cout'], g, x, w, relu)
            want = _round16(ref['gx'], nh_dtype(r['kind']))
            assert np.array_equal(gx, want), (M, relu, np.argwhere(gx != want)[:4].tolist())
            assert np.array_equal(dw, ref['dw']), (M, relu, np.argwhere(dw != ref['dw'])[:4].tolist())
            assert np.array_equal(db, ref['db']), (M, relu, db, ref['db'])


def test_narrow_head_bounded():
    _every_row(NH_IDS, _narrow_head_bounded_row)


def _narrow_head_bounded_row(rid):
    r = NH_FORMS[NH_IDS.index(rid)]
    u16, tiny = (0.0, 0.0) if r['kind'] == '32' else _u16()
    no = r['Cout']
    worst = [0.0, 0.0, 0.0]
    for M in r['Ms']:
        for relu in (0, 1):
            g, x, w = nh_operands(r['kind'], no, r['Cin'], M, False, relu)
            ref = reference_narrow_bwd(g[:, :no], x, w, relu)
            gx, dw, db = _nh_entry(r['kind'], no, g, x, w, relu)
            bx = no * U / (1 - no * U) * ref['mag_gx']
            bx = bx + u16 * (np.abs(ref['gx']) + bx) + tiny
            bounds = (bx, (M + 1) * U * ref['mag_dw'], M * U * ref['mag_db'])
            for i, (a, b, bd) in enumerate(zip((gx, dw, db), (ref['gx'], ref['dw'], ref['db']), bounds)):
                err = np.abs(a - b)
                assert (err <= bd).all(), (('gx', 'dw', 'db')[i], M, relu, float(np.nanmax(err / np.maximum(bd, 1e-300))))
                worst[i] = max(worst[i], float((err / np.maximum(bd, 1e-300)).max()))
    print(f'RATIO narrow {rid} gx {worst[0]:.3f} dw {worst[1]:.3f} db {worst[2]:.3f}')


def test_narrow_head_capped_grid_exact():
    """M = 32 768 + 37 rows at Cin = 1024, Cout = 6: 2048 blocks of 20 pixels, 407 of them beyond M; integers, so every output EQUALS
    the reference whatever the order of the 2048 x 6144 atomics."""
    kind, no, Cin, M = NH_BIG['kind'], NH_BIG['Cout'], NH_BIG['Cin'], NH_BIG_M
    g, x, w = nh_operands(kind, no, Cin, M, True)
    gx, dw, db = _nh_entry(kind, no, g, x, w, 1)
    g64, dwr = g[:, :no].astype(np.float64), np.zeros((no, Cin))
    for lo in range(0, M, 4096):
        ref = reference_narrow_bwd(g64[lo:lo + 4096], x[lo:lo + 4096], w, 1)
        assert np.array_equal(gx[lo:lo + 4096], ref['gx']), lo
        dwr += ref['dw']
    assert np.array_equal(dw, dwr) and np.array_equal(db, g64.sum(0))


def test_narrow_head_switches():
    """need_gx / need_dw / need_db off alone: None for itself, the other two bit-identical (integers); M = 0 returns zeros."""
    _every_row(NH_IDS, _narrow_head_switches_row)


def _narrow_head_switches_row(rid):
    from bonai_amd import kernels as K
    r = NH_FORMS[NH_IDS.index(rid)]
    M, no = r['Ms'][3], r['Cout']
    g, x, w = nh_operands(r['kind'], no, r['Cin'], M, True)
    gt, xt = _nh_tensors(r['kind'], g, x)
    wt = _dev(w)
    full = K.narrow_head_bwd(gt, xt, wt, relu_in=True)
    ref = reference_narrow_bwd(g[:, :no], x, w, 1)
    assert full[0].dtype == nh_dtype(r['kind']) and full[0].shape == xt.shape
    assert np.array_equal(full[0].permute(0, 2, 3, 1).reshape(M, -1).double().cpu().numpy(), _round16(ref['gx'], nh_dtype(r['kind'])))
    assert np.array_equal(full[1].double().cpu().numpy(), ref['dw']) and np.array_equal(full[2].double().cpu().numpy(), ref['db'])
    for off in range(3):
        need = [True] * 3
        need[off] = False
        part = K.narrow_head_bwd(gt, xt, wt, relu_in=True, need_gx=need[0], need_dw=need[1], need_db=need[2])
        assert part[off] is None and all(torch.equal(part[i], full[i]) for i in range(3) if i != off)
    gt0, xt0 = _nh_tensors(r['kind'], g[:0], x[:0])
    z = K.narrow_head_bwd(gt0, xt0, wt, relu_in=True)
    assert z[0].numel() == 0 and not z[1].any() and not z[2].any() and z[1].shape == (no, r['Cin']) and z[2].shape == (no,)


# ---- sampled_avg_factor ---------------------------------------------------------------------------------------------------------------
def test_sampled_avg_factor():
    _every_row(AVG_SHAPES, _sampled_avg_factor_shape)


def _sampled_avg_factor_shape(shape):
    from bonai_amd import kernels as K
    for fill in AVG_FILLS:
        pv, nv = avg_operands(shape, fill)
        want = reference_avg_factor(pv, nv)
        got = K.sampled_avg_factor(_dev(pv), _dev(nv))
        assert got.dtype == torch.float32 and got.shape == (1,) and float(got) == float(want), (fill, float(got), want)
        if fill != 'bytes':
            assert float(K.sampled_avg_factor(_dev(pv).bool(), _dev(nv).bool())) == float(want)
