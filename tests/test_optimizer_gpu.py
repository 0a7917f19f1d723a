"""GPU: the fused optimizer kernels of the config's optimizer -- loft_adamw_f32 (+ its device-side step count) and
loft_sgd_momentum_seg_f32 -- and ``Trainer(optimizer=..., paramwise_cfg=...)``.

Inputs, the float64 torch.optim references and the counted error bounds (K * 2^-24, derivation in that module's docstring) come from
tests/test_optimizer_cpu.py, which also shows that the inputs break the bound under each of three wrong AdamW formulas.

Sizes (test_optimizer_cpu.launch_passes mirrors the entry points' launch geometry; its own test pins what each size reaches):
  small, n = 4099: five workgroups, every 16-byte group in the single remainder pass, a 3-float tail; on views offset by one float
    everything goes through the scalar path.  Segment boundaries 8 and 512 lie inside the first workgroup's 1024-float span.
  big, n = 16 781 219: the grid is at its cap of 8192 workgroups, so every lane runs one iteration of the two-group unrolled body,
    lanes 0..999 the remainder pass, and 3 floats the tail.
"""
import pytest
import torch

from test_optimizer_cpu import (BETAS, BIG_ENDS, EPS, GSCALE, LR, MU, SMALL_ENDS, U, WD, K_ADAMW_P, K_SGD_P, bounds, f32, make_inputs,
                                reference)

pytestmark = pytest.mark.gpu


def _view(src, off):
    """A device copy of ``src`` that starts ``off`` floats into its allocation (off = 1: not 16-byte aligned)."""
    buf = torch.empty(src.numel() + off, dtype=torch.float32, device='cuda')
    v = buf[off:]
    v.copy_(src)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope='module')
def small():
    return make_inputs(SMALL_ENDS)


@pytest.fixture(scope='module')
def big():
    return make_inputs(BIG_ENDS)


def _table(inp, ones=False):
    from bonai_amd import kernels as K
    segs = [(e, 1.0 if ones else lm, 1.0 if ones else dm) for e, (lm, dm) in zip(inp['ends'], inp['mults'])]
    return K.SegmentTable(segs, inp['ends'][-1], 'cuda')


def _dev(inp, off, keys=('p', 'g', 'm', 'v')):
    return [_view(inp[k], off) for k in keys]


def _check(rule, inp, ref, got, steps=1):
    """|got - ref| <= the counted bound, element by element: p within K_P u (|p| + sum |dp|), m and v within K u |value|."""
    b = bounds(rule, inp, ref, steps)
    for k, t in got.items():
        err = (t.detach().cpu().double() - ref[k]).abs()
        worst = float((err / b[k].clamp_min(1e-300)).max())
        print(f'{rule} {k}: worst error / bound = {worst:.3f} over {t.numel()} elements, {steps} step(s)')
        assert bool((err <= b[k]).all()), (rule, k, worst)
    lm0 = [i for i, (lm, _) in enumerate(inp['mults']) if lm == 0.0]
    return lm0


def _adamw_steps(inp, off, steps, t0, max_norm, gfacs=None, ls_state=None, gscale=GSCALE, table=True):
    from bonai_amd import kernels as K
    p, g, m, v = _dev(inp, off)
    ss = inp['ss'].cuda()
    st = K.adamw_state_new(t0, *BETAS, 'cuda')
    tab = _table(inp) if table else None
    for t in range(steps):
        gt = g if gfacs is None else _view(inp['g'] * gfacs[t], off)
        K.adamw_(p, gt, m, v, ss, max_norm, LR, BETAS[0], BETAS[1], EPS, WD, st, grad_scale=gscale, table=tab, ls_state=ls_state)
        K.adamw_state_advance_(st, ss, *BETAS, skip_nonfinite=ls_state is not None)
    assert K.adamw_state_step(st) == t0 + steps
    return dict(p=p, m=m, v=v)


# ------------------------------------------------------------------ 1. AdamW against float64 torch.optim.AdamW

@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('max_norm', [100.0, 1.0, 0.0])          # above the norm (~5), below it (the clip applies), clip disabled
@pytest.mark.parametrize('t', [1, 3])
def test_adamw_one_step(small, off, max_norm, t):
    """grad_scale = 0.5; multipliers (1,1), (2,0), (0.1,1), (0,1), (1,1) on the five segments; one step at step count t."""
    ref = reference('AdamW', small, t0=t - 1, max_norm=max_norm)
    got = _adamw_steps(small, off, 1, t - 1, max_norm)
    for i in _check('AdamW', small, ref, got):
        a, b = ([0] + small['ends'])[i], small['ends'][i]
        assert torch.equal(got['p'][a:b].cpu(), small['p'][a:b])              # lr_mult = 0: p does not change at all
        assert not torch.equal(got['m'][a:b].cpu(), small['m'][a:b])           # ... while its moments do move
    assert not torch.equal(got['p'][:8].cpu(), small['p'][:8])


@pytest.mark.parametrize('off', [0, 1])
def test_adamw_three_consecutive_steps(small, off):
    gfacs = [1.0, 0.5, 2.0]                                                    # (powers of two: g * gfac is exact)
    ref = reference('AdamW', small, steps=3, max_norm=1.0, gfacs=gfacs)
    got = _adamw_steps(small, off, 3, 0, 1.0, gfacs=gfacs)
    _check('AdamW', small, ref, got, steps=3)


def test_adamw_unrolled_body_remainder_and_tail(big):
    ref = reference('AdamW', big, max_norm=100.0)
    got = _adamw_steps(big, 0, 1, 0, 100.0)
    for i in _check('AdamW', big, ref, got):
        a, b = ([0] + big['ends'])[i], big['ends'][i]
        assert torch.equal(got['p'][a:b].cpu(), big['p'][a:b])


def test_adamw_null_table_is_the_all_ones_table_and_padding_stays_zero(small):
    from bonai_amd import kernels as K
    inp = dict(small, p=small['p'].clone(), g=small['g'].clone(), m=small['m'].clone(), v=small['v'].clone())
    for k in 'pgmv':
        inp[k][504:512] = 0.0                                                  # an arena slot's padding: p = g = m = v = 0
    a = _adamw_steps(inp, 0, 1, 0, 1.0, table=False)
    p, g, m, v = _dev(inp, 0)
    st = K.adamw_state_new(0, *BETAS, 'cuda')
    K.adamw_(p, g, m, v, inp['ss'].cuda(), 1.0, LR, BETAS[0], BETAS[1], EPS, WD, st, grad_scale=GSCALE, table=_table(inp, ones=True))
    for k, t in (('p', p), ('m', m), ('v', v)):
        assert torch.equal(_bits(a[k]), _bits(t)), k
        assert torch.equal(t[504:512].cpu(), torch.zeros(8))
    assert K.adamw_state_step(st) == 0                                         # the wide kernel only reads the step state


# ------------------------------------------------------------------ 2. segmented SGD

@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('max_norm', [100.0, 1.0, 0.0])
def test_sgd_seg_null_and_all_ones_table_equal_the_plain_kernel_bit_for_bit(small, off, max_norm):
    from bonai_amd import kernels as K
    ss = small['ss'].cuda()
    p0, g, m0 = _dev(small, off, 'pgm')
    K.sgd_momentum_(p0, g, m0, ss, max_norm, LR, MU, WD, grad_scale=GSCALE)
    assert not torch.equal(p0.cpu(), small['p'])
    for tab in (None, _table(small, ones=True)):
        p, _, m = _dev(small, off, 'pgm')
        K.sgd_momentum_seg_(p, g, m, ss, max_norm, LR, MU, WD, grad_scale=GSCALE, nesterov=False, table=tab)
        assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(m), _bits(m0)), tab


def test_sgd_seg_null_table_equals_the_plain_kernel_through_the_unrolled_body(big):
    from bonai_amd import kernels as K
    ss = big['ss'].cuda()
    p0, g, m0 = _dev(big, 0, 'pgm')
    K.sgd_momentum_(p0, g, m0, ss, 100.0, LR, MU, WD, grad_scale=GSCALE)
    p, _, m = _dev(big, 0, 'pgm')
    K.sgd_momentum_seg_(p, g, m, ss, 100.0, LR, MU, WD, grad_scale=GSCALE, table=_table(big, ones=True))
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(m), _bits(m0))


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('nesterov', [True, False])
@pytest.mark.parametrize('max_norm', [1.0, 0.0])
def test_sgd_seg_multipliers_and_nesterov(small, off, nesterov, max_norm):
    from bonai_amd import kernels as K
    ref = reference('SGD', small, max_norm=max_norm, nesterov=nesterov)
    p, g, m = _dev(small, off, 'pgm')
    K.sgd_momentum_seg_(p, g, m, small['ss'].cuda(), max_norm, LR, MU, WD, grad_scale=GSCALE, nesterov=nesterov, table=_table(small))
    for i in _check('SGD', small, ref, dict(p=p, m=m)):
        a, b = ([0] + small['ends'])[i], small['ends'][i]
        assert torch.equal(p[a:b].cpu(), small['p'][a:b])
    if nesterov:                  # (the flag does something: outside the lr_mult = 0 segment the plain rule leaves the bound)
        plain = reference('SGD', small, max_norm=max_norm, nesterov=False)
        out = ((plain['p'] - ref['p']).abs() > bounds('SGD', small, ref)['p'])[:small['ends'][2]]
        assert float(out.double().mean()) > 0.5           # (gradients below ~1e-5 move p by less than the bound under either rule)


def test_sgd_seg_nesterov_unrolled_body_remainder_and_tail(big):
    from bonai_amd import kernels as K
    ref = reference('SGD', big, max_norm=100.0, nesterov=True)
    p, g, m = _dev(big, 0, 'pgm')
    K.sgd_momentum_seg_(p, g, m, big['ss'].cuda(), 100.0, LR, MU, WD, grad_scale=GSCALE, nesterov=True, table=_table(big))
    _check('SGD', big, ref, dict(p=p, m=m))


# ------------------------------------------------------------------ 3. the loss-scale form

N = SMALL_ENDS[-1]


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('where', [0, N // 2, N - 1])            # first element, 16-byte body, last element of the scalar tail
@pytest.mark.parametrize('bad', [float('inf'), float('nan'), 3e19])            # 3e19: finite, its square overflows fp32
def test_overflow_writes_nothing_and_the_next_step_never_saw_it(small, off, where, bad):
    from bonai_amd import kernels as K
    gh = small['g'].clone()
    gh[where] = bad
    gbad = _view(gh, off)
    ssbad = torch.zeros(1, device='cuda')
    K.sumsq_(gbad, ssbad)
    ss, tab = small['ss'].cuda(), _table(small)
    ls = K.loss_scale_state_pack(2.0).cuda()                                   # inv_world 1 / scale 2 = the grad_scale 0.5 of the reference
    # AdamW: one clean step (t = 1), the overflowing one, one more clean step (must be t = 2)
    p, g, m, v = _dev(small, off)
    st = K.adamw_state_new(0, *BETAS, 'cuda')

    def adam(gt, sst):
        K.adamw_(p, gt, m, v, sst, 1.0, LR, BETAS[0], BETAS[1], EPS, WD, st, grad_scale=1.0, table=tab, ls_state=ls)
        K.adamw_state_advance_(st, sst, *BETAS, skip_nonfinite=True)
    adam(g, ss)
    keep = [x.clone() for x in (p, m, v, st)]
    adam(gbad, ssbad)
    for x, y in zip((p, m, v, st), keep):
        assert torch.equal(_bits(x), _bits(y))                                 # p, m, v and the step words: bit-unchanged
    assert K.adamw_state_step(st) == 1
    adam(g, ss)
    assert K.adamw_state_step(st) == 2
    _check('AdamW', small, reference('AdamW', small, steps=2, max_norm=1.0), dict(p=p, m=m, v=v), steps=2)
    assert torch.equal(ls.cpu(), K.loss_scale_state_pack(2.0))                 # both launches only read the scaler's state
    # SGD (Nesterov, multipliers)
    p, g, m = _dev(small, off, 'pgm')
    sgd = lambda gt, sst: K.sgd_momentum_seg_(p, gt, m, sst, 1.0, LR, MU, WD, grad_scale=1.0, nesterov=True, table=tab, ls_state=ls)
    sgd(g, ss)
    keep = [x.clone() for x in (p, m)]
    sgd(gbad, ssbad)
    assert torch.equal(_bits(p), _bits(keep[0])) and torch.equal(_bits(m), _bits(keep[1]))
    sgd(g, ss)
    _check('SGD', small, reference('SGD', small, steps=2, max_norm=1.0, nesterov=True), dict(p=p, m=m), steps=2)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('max_norm', [100.0, 1.0, 0.0])
def test_loss_scale_form_is_bit_identical_to_static_at_power_of_two_scale(small, off, max_norm):
    from bonai_amd import kernels as K
    ls = K.loss_scale_state_pack(512.0).cuda()
    static = _adamw_steps(small, off, 1, 0, max_norm, gscale=0.25 / 512.0)
    scaled = _adamw_steps(small, off, 1, 0, max_norm, gscale=0.25, ls_state=ls)
    assert all(torch.equal(_bits(static[k]), _bits(scaled[k])) for k in 'pmv')
    assert not torch.equal(static['p'].cpu(), small['p'])
    ss, tab = small['ss'].cuda(), _table(small)
    p1, g, m1 = _dev(small, off, 'pgm')
    K.sgd_momentum_seg_(p1, g, m1, ss, max_norm, LR, MU, WD, grad_scale=0.25 / 512.0, nesterov=True, table=tab)
    p2, _, m2 = _dev(small, off, 'pgm')
    K.sgd_momentum_seg_(p2, g, m2, ss, max_norm, LR, MU, WD, grad_scale=0.25, nesterov=True, table=tab, ls_state=ls)
    assert torch.equal(_bits(p1), _bits(p2)) and torch.equal(_bits(m1), _bits(m2))


# ------------------------------------------------------------------ 4.-6. trainer level: a toy module with a norm layer and biases

class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.backbone = torch.nn.Linear(4, 3, bias=False)
        self.fc = torch.nn.Linear(5, 3)
        self.norm = torch.nn.LayerNorm(6)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)

    def train_step(self, data):
        loss = sum((p * data[n]).sum() for n, p in self.named_parameters())
        return dict(loss=loss, log_vars={}, num_samples=1)


PARAMWISE = dict(norm_decay_mult=0., bias_lr_mult=2., custom_keys={'backbone': dict(lr_mult=f32(0.1))})
ADAMW = dict(type='AdamW', lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
SGD_NEST = dict(type='SGD', lr=LR, momentum=MU, weight_decay=f32(1e-4), nesterov=True)


def _toy_data(step):
    """Positive, step-dependent gradients (the loss is linear in the parameters): 0.5 .. 2 times 1, 0.5, 2, 1."""
    gen = torch.Generator().manual_seed(17)
    fac = [1.0, 0.5, 2.0, 1.0][step]
    return {n: ((0.5 + 1.5 * torch.rand(p.shape, generator=gen)) * fac).cuda() for n, p in _Toy().named_parameters()}


def _toy_trainer(optimizer, **kw):
    from bonai_amd.engine import Trainer
    return Trainer(_Toy().cuda(), optimizer=optimizer, paramwise_cfg=PARAMWISE, **kw)


def _torch_optimizer(tr, optimizer, params):
    """The float64 torch optimizer mmcv would build: one param group per parameter with its own lr / weight_decay."""
    opt = dict(optimizer)
    cls = getattr(torch.optim, opt.pop('type'))
    groups = []
    for (n, _), q in zip(tr.model.named_parameters(), params):
        lm, dm = tr.optim.mult_of(n)
        groups.append(dict(params=[q], lr=opt['lr'] * lm, weight_decay=opt['weight_decay'] * dm))
    return cls(groups, **opt)


@pytest.mark.parametrize('optimizer,k', [(ADAMW, K_ADAMW_P), (SGD_NEST, K_SGD_P)], ids=['AdamW', 'SGD-nesterov'])
def test_trainer_follows_float64_torch_optim(optimizer, k):
    """After each step the arena's gradients drive torch.optim on a float64 CPU copy; the parameters agree within the one-step bound
    times the step count.  max_norm=None (no clip): the gradient the kernel applies is the arena's, exactly."""
    tr = _toy_trainer(optimizer, max_norm=None)
    assert tr.seg_table is not None and len(tr.seg_table) >= 3 and (tr.exp_avg_sq is not None) == (optimizer['type'] == 'AdamW')
    params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in tr.model.parameters()]
    p0 = [q.detach().clone() for q in params]
    ref = _torch_optimizer(tr, optimizer, params)
    dp_abs = [torch.zeros_like(q) for q in params]
    for step in range(4):
        tr.train_step(_toy_data(step))
        before = [q.detach().clone() for q in params]
        for q, p in zip(params, tr.model.parameters()):
            q.grad = p.grad.detach().cpu().double().clone()                    # (views of arena.grad)
            assert float(q.grad.min()) > 0
        ref.step()
        for i, (q, p) in enumerate(zip(params, tr.model.parameters())):
            dp_abs[i] += (q.detach() - before[i]).abs()
            bound = (step + 1) * k * U * (p0[i].abs() + dp_abs[i])
            err = (p.detach().cpu().double() - q.detach()).abs()
            print(f"{optimizer['type']} step {step + 1} parameter {i}: worst error / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (step, i)
    assert all(float(d.min()) > 0 for d in dp_abs)                             # every parameter moved


def test_checkpoint_resumes_bit_for_bit_and_loads_into_torch_adamw():
    a = _toy_trainer(ADAMW, max_norm=35.0, loss_scale=dict(init_scale=4, growth_interval=10 ** 9))
    for step in range(2):
        a.train_step(_toy_data(step))
    sd = a.optimizer_state_dict()
    weights = a.arena.data.clone()
    for step in (2, 3):
        a.train_step(_toy_data(step))
    b = _toy_trainer(ADAMW, max_norm=35.0, loss_scale=dict(init_scale=4, growth_interval=10 ** 9))
    b.arena.data.copy_(weights)
    b.load_optimizer_state(sd)
    assert b.iter == 2 and b.loss_scale_state() == sd['loss_scaler']
    for step in (2, 3):
        b.train_step(_toy_data(step))
    assert torch.equal(_bits(a.arena.data), _bits(b.arena.data)) and torch.equal(_bits(a.arena.momentum), _bits(b.arena.momentum))
    assert torch.equal(_bits(a.exp_avg_sq), _bits(b.exp_avg_sq)) and torch.equal(_bits(a.opt_state), _bits(b.opt_state))
    # torch.optim.AdamW.state_dict() layout: a real AdamW over the same parameters, grouped as mmcv groups them, takes it
    params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in a.model.parameters()]
    real = _torch_optimizer(a, ADAMW, params)
    assert len(sd['param_groups']) == len(params) and [g['params'] for g in sd['param_groups']] == [[i] for i in range(len(params))]
    for g, rg in zip(sd['param_groups'], real.state_dict()['param_groups']):
        assert set(g) == set(rg) and g['lr'] == rg['lr'] and g['weight_decay'] == rg['weight_decay'] and tuple(g['betas']) == BETAS
    real.load_state_dict({k: sd[k] for k in ('state', 'param_groups')})
    for i, q in enumerate(params):
        st = real.state[q]
        assert float(st['step']) == 2.0
        assert torch.equal(st['exp_avg'], sd['state'][i]['exp_avg']) and torch.equal(st['exp_avg_sq'], sd['state'][i]['exp_avg_sq'])
        assert st['exp_avg'].shape == q.shape and float(st['exp_avg_sq'].min()) > 0
    for q in params:
        q.grad = torch.ones_like(q)
    real.step()                                                                 # ... and can step with it
    # the other rule's state is refused, both ways
    s = _toy_trainer(SGD_NEST)
    s.train_step(_toy_data(0))
    with pytest.raises(RuntimeError, match='SGD.*AdamW'):
        b.load_optimizer_state(s.optimizer_state_dict())
    with pytest.raises(RuntimeError, match='AdamW.*SGD'):
        s.load_optimizer_state(sd)
    assert s.optimizer_state_dict()['param_groups'][0]['nesterov'] is True


def test_plain_trainer_calls_only_the_entry_points_it_always_called(monkeypatch):
    from bonai_amd import kernels as K
    from bonai_amd.engine import Trainer
    calls = []
    for name in ('sgd_momentum_', 'sgd_momentum_scaled_', 'loss_scale_update_', 'sumsq_', 'sgd_momentum_seg_', 'adamw_',
                 'adamw_state_advance_', 'adamw_state_new'):
        def wrap(*a, _f=getattr(K, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(K, name, wrap)
    for scale, want in ((512.0, ['sumsq_', 'sgd_momentum_']), ('dynamic', ['sumsq_', 'sgd_momentum_scaled_', 'loss_scale_update_'])):
        for kw in ({}, dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=1e-4))):    # the same SGD, from a config
            del calls[:]
            tr = Trainer(_Toy().cuda(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=35.0, loss_scale=scale, **kw)
            before = tr.arena.data.clone()
            tr.train_step(_toy_data(0))
            tr.train_step(_toy_data(1))
            assert calls == want * 2, (scale, kw, calls)
            assert tr.exp_avg_sq is None and tr.opt_state is None and tr.seg_table is None
            assert not torch.equal(tr.arena.data, before)
            sd = tr.optimizer_state_dict()
            assert len(sd['param_groups']) == 1 and set(sd['state'][0]) == {'momentum_buffer'}
    del calls[:]
    _toy_trainer(ADAMW).train_step(_toy_data(0))                               # (the wrappers do count: the AdamW path shows up)
    assert calls == ['adamw_state_new', 'sumsq_', 'adamw_', 'adamw_state_advance_']
