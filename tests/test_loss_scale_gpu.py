"""GPU: dynamic loss scaling decided on the device -- loft_sgd_momentum_scaled_f32 + loft_loss_scale_update (include/loft_hip.h) and
``Trainer(loss_scale='dynamic' | dict)``.  An extension: the reference's Fp16OptimizerHook (mmdet/core/fp16/hooks.py:64-96) is
static-only; the rule checked here is torch.amp.GradScaler's plus the min / max clamps.

Kernel level: flat fp32 arenas of n = 4099 (a float4 body + a 3-element tail), each case also on views offset by one float (the
unaligned, all-scalar path).  Trainer level: a one-parameter toy module, and one real binary16 overflow on the synthetic-weight R50.
"""
import os
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4099
LR, MU, WD = 0.01, 0.9, 1e-4


def _view(src, off):
    """A device copy of ``src`` that starts ``off`` floats into its allocation (off = 1: not 16-byte aligned)."""
    buf = torch.empty(src.numel() + off, dtype=torch.float32, device='cuda')
    v = buf[off:]
    v.copy_(src)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


@pytest.fixture(scope='module')
def arenas():
    """Random p / g / m on the host, made once; g is a gradient under loss scale 512 (unscaled norm ~ sqrt(n) = 64)."""
    gen = torch.Generator().manual_seed(11)
    return dict(p=torch.randn(N, generator=gen), g=torch.randn(N, generator=gen) * 512.0, m=torch.randn(N, generator=gen) * 0.1)


def _sumsq(g):
    from bonai_amd import kernels as K
    ss = torch.zeros(1, dtype=torch.float32, device='cuda')
    K.sumsq_(g, ss)
    return ss


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('max_norm', [1000.0, 10.0, 0.0])      # above the norm (~64), below it (the clip applies), clip disabled
def test_scaled_sgd_is_bit_identical_to_static_at_power_of_two_scale(arenas, off, max_norm):
    from bonai_amd import kernels as K
    g = _view(arenas['g'], off)
    ss = _sumsq(g)
    norm = float(ss.cpu()[0]) ** 0.5 / 512.0
    assert (norm > max_norm) == (max_norm == 10.0) or max_norm == 0.0
    p1, m1 = _view(arenas['p'], off), _view(arenas['m'], off)
    K.sgd_momentum_(p1, g, m1, ss, max_norm, LR, MU, WD, grad_scale=1.0 / 512.0)
    p2, m2 = _view(arenas['p'], off), _view(arenas['m'], off)
    state = K.loss_scale_state_pack(512.0).cuda()
    K.sgd_momentum_scaled_(p2, g, m2, ss, max_norm, LR, MU, WD, 1.0, state)
    assert not torch.equal(p1.cpu(), arenas['p'])                  # (a step was taken)
    assert torch.equal(_bits(p1), _bits(p2)) and torch.equal(_bits(m1), _bits(m2))
    assert torch.equal(state.cpu(), K.loss_scale_state_pack(512.0))  # the SGD launch only reads the state


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('where', [0, N // 2, N - 1])            # first element, float4 body, last element of the scalar tail
@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan'), 3e19])     # 3e19: finite, its square overflows fp32
def test_overflow_skips_the_whole_update_and_backs_off(arenas, off, where, bad):
    from bonai_amd import kernels as K
    gh = arenas['g'].clone()
    gh[where] = bad
    g = _view(gh, off)
    ss = _sumsq(g)
    p, m = _view(arenas['p'], off), _view(arenas['m'], off)
    p0, m0 = p.clone(), m.clone()
    state = K.loss_scale_state_pack(512.0, good_steps=5, skipped=0).cuda()
    K.sgd_momentum_scaled_(p, g, m, ss, 35.0, LR, MU, WD, 1.0, state)
    assert torch.equal(_bits(p), _bits(p0)) and torch.equal(_bits(m), _bits(m0))
    K.loss_scale_update_(state, ss, 1.0, 2.0, 0.5, 2000, 1.0, 2.0 ** 24)
    st = K.loss_scale_state_unpack(state)
    assert st['scale'] == 256.0 and st['good_steps'] == 0 and st['skipped'] == 1 and st['last_skipped'] is True
    assert not torch.isfinite(torch.tensor(st['grad_norm']))     # the recorded norm of a skipped step is non-finite as it stands


def _rule(scale, good, skipped, overflow, growth, backoff, interval, lo, hi):
    """torch.amp.GradScaler's update plus the clamps, in plain Python.  Every scale here is a power of two: exact in fp32."""
    if overflow:
        return max(scale * backoff, lo), 0, skipped + 1
    good += 1
    if good == interval:
        return min(scale * growth, hi), 0, skipped
    return scale, good, skipped


def _overflow_sequence(seed, p_overflow, steps=40):
    rnd = random.Random(seed)
    return [1 if rnd.random() < p_overflow else 0 for _ in range(steps)]


def test_plain_python_rule_agrees_with_torch_amp_update_scale():
    """The reference rule of the next test against torch's own kernel, which the installed torch runs on CPU tensors (no clamps in
    torch: the sequence stays inside the bounds)."""
    seq = _overflow_sequence(5, 0.3)
    scale_t, track_t = torch.tensor([1024.0]), torch.tensor([0], dtype=torch.int32)
    scale, good, skipped = 1024.0, 0, 0
    for ov in seq:
        torch._amp_update_scale_(scale_t, track_t, torch.tensor([float(ov)]), 2.0, 0.5, 3)
        scale, good, skipped = _rule(scale, good, skipped, ov, 2.0, 0.5, 3, 2.0 ** -100, 2.0 ** 100)
        assert float(scale_t) == scale and int(track_t) == good


@pytest.mark.parametrize('start,p_overflow,seed,bound', [(4.0, 0.35, 2, 'min'), (2.0 ** 23, 0.15, 2, 'max')])
def test_update_rule_matches_gradscaler_with_clamps_at_every_step(start, p_overflow, seed, bound):
    from bonai_amd import kernels as K
    growth, backoff, interval, lo, hi = 2.0, 0.5, 3, 1.0, 2.0 ** 24
    seq = _overflow_sequence(seed, p_overflow)
    assert 0 < sum(seq) < len(seq)
    want, clamped, (scale, good, skipped) = [], 0, (start, 0, 0)
    for ov in seq:
        if (bound == 'min' and ov and scale * backoff < lo) or (bound == 'max' and not ov and good + 1 == interval and scale * growth > hi):
            clamped += 1
        scale, good, skipped = _rule(scale, good, skipped, ov, growth, backoff, interval, lo, hi)
        want.append((scale, good, skipped, bool(ov)))
    assert clamped >= 2 and len({w[0] for w in want}) >= 3, 'the sequence must grow, back off and run into the clamp'
    state = K.loss_scale_state_pack(start).cuda()
    clean, over = torch.full((1,), 4.0, device='cuda'), torch.full((1,), float('inf'), device='cuda')
    hist = torch.zeros(len(seq), K.LS_WORDS, dtype=torch.float32, device='cuda')
    for i, ov in enumerate(seq):
        K.loss_scale_update_(state, over if ov else clean, 1.0, growth, backoff, interval, lo, hi)
        hist[i].copy_(state)
    hist = hist.cpu()
    for i, w in enumerate(want):
        st = K.loss_scale_state_unpack(hist[i])
        assert (st['scale'], st['good_steps'], st['skipped'], st['last_skipped']) == w, (i, st, w)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('inv_world', [1.0, 0.25])
def test_recorded_grad_norm_is_the_unscaled_norm(arenas, off, inv_world):
    """One fp32 sum of 4099 squares (tree-shaped inside the kernel) is far inside 1e-5 relative; sqrt, one product and one division
    add three roundings of 2^-24 each."""
    from bonai_amd import kernels as K
    g = _view(arenas['g'], off)
    ss = _sumsq(g)
    state = K.loss_scale_state_pack(512.0).cuda()
    K.loss_scale_update_(state, ss, inv_world, 2.0, 0.5, 2000, 1.0, 2.0 ** 24)
    st = K.loss_scale_state_unpack(state)
    want = float(arenas['g'].double().norm()) * inv_world / 512.0
    assert st['last_skipped'] is False and st['good_steps'] == 1 and st['scale'] == 512.0
    assert abs(st['grad_norm'] - want) <= 1e-5 * want, (st['grad_norm'], want)


# ------------------------------------------------------------------ trainer level: a toy module

class _Toy(torch.nn.Module):
    def __init__(self, n=37):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, n))

    def train_step(self, data):
        return dict(loss=(self.w * data['x']).sum(), log_vars={}, num_samples=1)


def _toy_trainer(loss_scale):
    from bonai_amd.engine import Trainer
    return Trainer(_Toy().cuda(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=35.0, loss_scale=loss_scale)


def _toy_x(spike=None):
    x = torch.linspace(0.5, 2.0, 37, device='cuda')
    if spike is not None:
        x[11] = spike
    return dict(x=x)


def test_toy_dynamic_equals_static_then_skips_then_applies():
    dyn, sta = _toy_trainer(dict(init_scale=512, growth_interval=10 ** 9)), _toy_trainer(512.0)
    assert dyn.loss_scale is None and sta.scaler is None and sta.scale_state is None
    init = dyn.arena.data.clone()
    for _ in range(3):
        dyn.train_step(_toy_x())
        sta.train_step(_toy_x())
    assert torch.equal(_bits(dyn.arena.data), _bits(sta.arena.data)) and torch.equal(_bits(dyn.arena.momentum), _bits(sta.arena.momentum))
    assert not torch.equal(dyn.arena.data, init)                # (steps were taken)
    st = dyn.loss_scale_state()
    assert st['scale'] == 512.0 and st['good_steps'] == 3 and st['skipped'] == 0 and st['last_skipped'] is False
    ref = sta.loss_scale_state()
    assert ref['scale'] == 512.0 and ref['skipped'] == 0 and ref['last_skipped'] is False
    assert abs(st['grad_norm'] - ref['grad_norm']) <= 1e-6 * ref['grad_norm']
    assert abs(ref['grad_norm'] - float(_toy_x()['x'].double().norm())) <= 1e-5 * ref['grad_norm']

    tr = _toy_trainer(dict(init_scale=4, growth_interval=10 ** 9))
    tr.train_step(_toy_x())                                     # one applied step: the momentum is not zero any more
    data0, mom0 = tr.arena.data.clone(), tr.arena.momentum.clone()
    assert float(mom0.abs().sum()) > 0
    tr.train_step(_toy_x(spike=3e38))                           # 4 * 3e38 is inf in fp32
    assert torch.isinf(tr.arena.grad).any()
    assert torch.equal(_bits(tr.arena.data), _bits(data0)) and torch.equal(_bits(tr.arena.momentum), _bits(mom0))
    st = tr.loss_scale_state()
    assert st['scale'] == 2.0 and st['skipped'] == 1 and st['last_skipped'] is True and st['good_steps'] == 0
    assert tr.iter == 2                                         # the schedule does not stall on a skipped step
    tr.train_step(_toy_x())
    assert not torch.equal(tr.arena.data, data0) and torch.isfinite(tr.arena.data).all()
    st = tr.loss_scale_state()
    assert st['scale'] == 2.0 and st['skipped'] == 1 and st['last_skipped'] is False and st['good_steps'] == 1 and tr.iter == 3


def test_static_path_never_touches_the_dynamic_kernels(monkeypatch):
    from bonai_amd import kernels as K

    def boom(*a, **k):
        raise AssertionError('the static loss-scale path called a dynamic-scaler kernel')
    monkeypatch.setattr(K, 'sgd_momentum_scaled_', boom)
    monkeypatch.setattr(K, 'loss_scale_update_', boom)
    tr = _toy_trainer(512.0)
    before = tr.arena.data.clone()
    tr.train_step(_toy_x())
    assert not torch.equal(tr.arena.data, before) and torch.isfinite(tr.arena.data).all()
    assert 'loss_scaler' not in tr.optimizer_state_dict()
    with pytest.raises(AssertionError):
        _toy_trainer('dynamic').train_step(_toy_x())          # (the patch is in force: the dynamic path does call them)


def test_loss_scaler_state_travels_with_the_optimizer_state():
    spec = dict(init_scale=4, growth_interval=10 ** 9)
    tr = _toy_trainer(spec)
    tr.train_step(_toy_x())
    tr.train_step(_toy_x(spike=3e38))
    want = tr.loss_scale_state()
    assert want['skipped'] == 1 and want['scale'] == 2.0
    sd = tr.optimizer_state_dict()
    assert sd['loss_scaler'] == want
    fresh = _toy_trainer(spec)
    fresh.load_optimizer_state(sd)
    assert fresh.loss_scale_state() == want and fresh.iter == 2
    assert torch.equal(fresh.arena.momentum, tr.arena.momentum)
    plain = {k: v for k, v in sd.items() if k != 'loss_scaler'}  # a reference-format SGD state: no such key
    other = _toy_trainer(spec)
    other.load_optimizer_state(plain)
    st = other.loss_scale_state()
    assert st['scale'] == 4.0 and st['skipped'] == 0 and st['good_steps'] == 0
    static = _toy_trainer(4.0)
    static.load_optimizer_state(sd)                             # a static trainer ignores the entry
    assert static.loss_scale_state()['scale'] == 4.0


# ------------------------------------------------------------------ trainer level: a real binary16 overflow

@pytest.fixture()
def fp16_first_sampler():
    from bonai_amd import lib as L
    from bonai_amd.loft.core import RandomSampler
    prev, prev_mode = L.set_act16(torch.float16), RandomSampler.choice_mode
    RandomSampler.choice_mode = 'first'
    yield
    RandomSampler.choice_mode = prev_mode
    L.set_act16(prev)


def test_real_fp16_overflow_is_skipped_until_the_scale_fits(fp16_first_sampler):
    """At scale 2^24 the backward seed alone exceeds binary16's 65504: the first step must be skipped.  The scale halves per skipped
    step, so a step must apply within log2(2^24 / min_scale) = 24 steps (the static test shows the path works at 512)."""
    from bonai_amd.config import Config
    from bonai_amd.engine import Trainer
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().train()
    data = make_batch(1, 256, 6, device='cuda')
    tr = Trainer(m, lr=1e-3, loss_scale=dict(init_scale=2 ** 24, growth_interval=10 ** 9))
    data0, mom0 = tr.arena.data.clone(), tr.arena.momentum.clone()
    tr.train_step(data)
    st = tr.loss_scale_state()
    assert torch.equal(_bits(tr.arena.data), _bits(data0)) and torch.equal(_bits(tr.arena.momentum), _bits(mom0))
    assert st['last_skipped'] is True and st['skipped'] == 1 and st['scale'] == 2.0 ** 23
    steps = 1
    while st['last_skipped'] and steps < 24:
        tr.train_step(data)
        steps += 1
        st = tr.loss_scale_state()
    print(f'first applied step: #{steps}, scale {st["scale"]}, skipped {st["skipped"]}, grad_norm {st["grad_norm"]}')
    assert st['last_skipped'] is False, f'no step applied within {steps} steps: {st}'
    assert torch.isfinite(tr.arena.data).all() and not torch.equal(tr.arena.data, data0)
    mant, _ = torch.frexp(torch.tensor(st['scale']))
    assert float(mant) == 0.5 and 1.0 <= st['scale'] <= 2.0 ** 23       # a power of two
    assert st['skipped'] + st['good_steps'] == steps == tr.iter and st['good_steps'] == 1
    assert st['scale'] == 2.0 ** (24 - st['skipped'])
