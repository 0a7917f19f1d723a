"""CPU: the optimizer of the config (bonai_amd/optim.py) -- parsing, mmcv's paramwise rule on the headline model, segment merging,
tools/train.py's trainer arguments -- and the inputs, float64 references and error bounds that tests/test_optimizer_gpu.py holds
the fused kernels (loft_adamw_f32, loft_sgd_momentum_seg_f32) to.

The reference is torch.optim.AdamW / torch.optim.SGD on the CPU in float64, one param group per segment, fed the fp32 inputs exactly
(every hyper-parameter below is an fp32-representable number; the betas are doubles on both sides).  The bound counts the kernel's own
fp32 roundings, u = 2^-24 per operation (bonai_amd/csrc/elementwise.hip is built without fast-math: division and square root are
correctly rounded; contraction into FMA only removes roundings):

  prologue   s = clip * gscale, clip = max_norm / (sqrt(ss) * gscale + 1e-6): sqrt, product, sum, quotient, product      5u
  gs = g * s                                                                                                              6u
  AdamW  m = b1*m + (1-b1)*gs   b1, 1-b1 rounded once each from the double (1u): terms 2u and 1+6+1 = 8u, the sum +1     9u   K_M = 10
         v = b2*v + (1-b2)*gs^2 gs^2 13u, times (1-b2) 15u, the sum +1                                                  16u   K_V = 17
         denom = sqrt(v)*rbc2 + eps   sqrt 16/2+1 = 9u, rbc2 (1u, rounded once from the double) and product 11u, sum     12u
         q = m / denom                9 + 12 + 1                                                                        22u
         step = lr*lr_mult*inv_bc1    product 1u, inv_bc1 1u, product 1u                                                 3u
         dp = step * q                22 + 3 + 1 = 26u of |dp|;  p*decay: decay = 1 - lr*wd 1u, product 1u = 2u of |p|;
         p - dp: 1u of |p| + |dp|     =>  27u * |dp| + 3u * |p|                                                              K_P = 28
  SGD    d = gs + wd*wd_mult*p  terms 6u and 2u, sum +1                                                                  7u
         m = mu*m + d           mu 1u, product 1u, sum +1 over max(2, 7)                                                 8u   K_M = 9
         Nesterov d + mu*m      max(7, 8+2) + 1 = 11u; times lr*lr_mult 13u; p - ...: +1u                                14u   K_P = 15
Each K carries one unit for the second-order terms.  The m / d sums are bounded relative to their VALUE only when their terms
do not cancel, so the inputs give p, g and m one sign per element (a momentum that agrees with its gradient).  T consecutive steps:
T times the one-step bound, with |dp| summed over the steps (the relative errors of m and v grow by at most their one-step figure
per step).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
K_ADAMW_P, K_ADAMW_M, K_ADAMW_V = 28, 10, 17
K_SGD_P, K_SGD_M = 15, 9
assert max(K_ADAMW_P, K_ADAMW_M, K_ADAMW_V, K_SGD_P, K_SGD_M) <= 32


def f32(x):
    return float(np.float32(x))


LR, WD, EPS, BETAS, MU = f32(0.01), f32(0.05), f32(1e-8), (0.9, 0.999), f32(0.9)
GSCALE = 0.5
MULTS = [(1.0, 1.0), (2.0, 0.0), (f32(0.1), 1.0), (0.0, 1.0), (1.0, 1.0), (2.0, 0.0)]

# ---- launch geometry of the entry points: ew_grid(n / 4) = min(ceil(n/4 / 256), 8192) workgroups of 256 lanes, one 16-byte group
# per lane and pass.  The two-groups-per-iteration body runs for a lane only if i + stride < n/4, the single remainder pass if then
# i < n/4 is left over, the scalar tail for the n % 4 last floats (or for everything when a base pointer is not 16-byte aligned).
GRID_CAP, LANES = 8192, 256


def launch_passes(n, aligned=True):
    n4 = n // 4 if aligned else 0
    stride = min(max((n // 4 + LANES - 1) // LANES, 1), GRID_CAP) * LANES
    unrolled = remainder = False
    for t0 in (0, stride - 1):                          # the kernel's loops, for the first and the last lane of the grid
        i = t0
        while i + stride < n4:
            unrolled, i = True, i + 2 * stride
        remainder = remainder or i < n4
    return dict(unrolled=unrolled, remainder=remainder, tail=n - 4 * n4 > 0)


# small: one workgroup-span (1024 floats) holds the boundaries 8 and 512; 4099 = 1024 groups + a 3-float tail, five workgroups
SMALL_ENDS = [8, 512, 1536, 3584, 4099]
# big: the grid is capped (stride = 8192 * 256 groups), every lane runs ONE two-group iteration, lanes 0..999 the remainder pass,
# three floats the tail; the first workgroup's span again holds the boundaries 8 and 512
BIG_N = 4 * (2 * GRID_CAP * LANES + 1000) + 3
BIG_ENDS = [8, 512, 1536, 4_000_000, 12_000_008, BIG_N]


def test_the_chosen_sizes_reach_every_pass_of_the_kernel():
    assert launch_passes(SMALL_ENDS[-1]) == dict(unrolled=False, remainder=True, tail=True)
    assert launch_passes(SMALL_ENDS[-1], aligned=False) == dict(unrolled=False, remainder=False, tail=True)
    assert launch_passes(BIG_N) == dict(unrolled=True, remainder=True, tail=True)
    n4, stride = BIG_N // 4, GRID_CAP * LANES
    assert n4 == 2 * stride + 1000 and BIG_N % 4 == 3               # written out: [0, 2*stride) unrolled, 1000 groups remain
    for ends in (SMALL_ENDS, BIG_ENDS):
        assert ends[0] == 8 and all(e % 8 == 0 for e in ends[:-1]) and ends[1] < 4 * LANES and len(ends) <= len(MULTS)


def make_inputs(ends, seed=3):
    """p, g, m, v as fp32 CPU tensors: |g| log-uniform over 1e-8 .. 1 (eps next to sqrt(v) matters at the small end), m and v a
    plausible Adam state of such gradients (m ~ g, v ~ g^2), p of size 0.1 .. 1; p, g, m share one sign per element."""
    n = ends[-1]
    gen = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8 - 8)
    g = (sign * mag).float()
    p = sign * (0.1 + 0.9 * torch.rand(n, generator=gen))
    m = (sign * mag * (0.2 + 0.8 * torch.rand(n, generator=gen, dtype=torch.float64))).float()
    v = (mag * mag * (0.2 + 0.8 * torch.rand(n, generator=gen, dtype=torch.float64))).float()
    ss = torch.tensor([float((g.double() ** 2).sum())], dtype=torch.float32)      # the fp32 scalar the kernels are handed
    return dict(p=p, g=g, m=m, v=v, ss=ss, ends=list(ends), mults=MULTS[:len(ends)])


def grad_factor(ss, max_norm, gscale):
    """clip * grad_scale in float64 from the fp32 sum of squares (torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6))."""
    clip = 1.0
    if max_norm > 0:
        norm = float(ss.double().sqrt()) * gscale
        if norm > max_norm:
            clip = max_norm / (norm + 1e-6)
    return clip * gscale


def _segments(inp, t):
    return [t[a:b] for a, b in zip([0] + inp['ends'][:-1], inp['ends'])]


def reference(rule, inp, steps=1, t0=0, max_norm=0.0, gscale=GSCALE, gfacs=None, nesterov=False, table=True):
    """float64 torch.optim over one param group per segment -> dict(p, m[, v], dp_abs): dp_abs is sum |p_t - p_(t-1)|.
    gfacs: per-step multipliers of g (consecutive steps see g * gfacs[t]); t0: steps already applied (AdamW's state step)."""
    gfacs = gfacs or [1.0] * steps
    s = grad_factor(inp['ss'], max_norm, gscale)
    mults = inp['mults'] if table else [(1.0, 1.0)] * len(inp['ends'])
    params = [torch.nn.Parameter(x.double().clone()) for x in _segments(inp, inp['p'])]
    groups = [dict(params=[q], lr=LR * lm, weight_decay=WD * dm) for q, (lm, dm) in zip(params, mults)]
    if rule == 'AdamW':
        opt = torch.optim.AdamW(groups, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, amsgrad=False, foreach=False)
        for q, m, v in zip(params, _segments(inp, inp['m']), _segments(inp, inp['v'])):
            opt.state[q] = dict(step=torch.tensor(float(t0), dtype=torch.float64), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    else:
        opt = torch.optim.SGD(groups, lr=LR, momentum=MU, weight_decay=WD, nesterov=nesterov, foreach=False)
        for q, m in zip(params, _segments(inp, inp['m'])):
            opt.state[q] = dict(momentum_buffer=m.double().clone())
    dp_abs = torch.zeros(inp['ends'][-1], dtype=torch.float64)
    for t in range(steps):
        before = torch.cat([q.detach().clone() for q in params])
        for q, g in zip(params, _segments(inp, inp['g'])):
            q.grad = g.double() * (s * gfacs[t])
        opt.step()
        dp_abs += (torch.cat([q.detach() for q in params]) - before).abs()
    out = dict(p=torch.cat([q.detach() for q in params]), dp_abs=dp_abs)
    if rule == 'AdamW':
        out['m'] = torch.cat([opt.state[q]['exp_avg'] for q in params])
        out['v'] = torch.cat([opt.state[q]['exp_avg_sq'] for q in params])
    else:
        out['m'] = torch.cat([opt.state[q]['momentum_buffer'] for q in params])
    return out


def bounds(rule, inp, ref, steps=1):
    kp, km = (K_ADAMW_P, K_ADAMW_M) if rule == 'AdamW' else (K_SGD_P, K_SGD_M)
    b = dict(p=steps * kp * U * (inp['p'].double().abs() + ref['dp_abs']), m=steps * km * U * ref['m'].abs())
    if rule == 'AdamW':
        b['v'] = steps * K_ADAMW_V * U * ref['v'].abs()
    return b


def _adamw_formula(inp, t, max_norm, wrong=None):
    """One AdamW step at step count t in float64, written out; ``wrong`` selects one of the three classic mistakes."""
    s = grad_factor(inp['ss'], max_norm, GSCALE)
    lm = torch.cat([torch.full((b - a,), m[0], dtype=torch.float64) for a, b, m in zip([0] + inp['ends'][:-1], inp['ends'], inp['mults'])])
    dm = torch.cat([torch.full((b - a,), m[1], dtype=torch.float64) for a, b, m in zip([0] + inp['ends'][:-1], inp['ends'], inp['mults'])])
    p, g, m, v = inp['p'].double(), inp['g'].double() * s, inp['m'].double(), inp['v'].double()
    lr, wd = LR * lm, WD * dm
    if wrong == 'coupled_decay':
        g = g + wd * p
    else:
        p = p * (1 - lr * wd)
    m = BETAS[0] * m + (1 - BETAS[0]) * g
    v = BETAS[1] * v + (1 - BETAS[1]) * g * g
    bc1, bc2 = (1.0, 1.0) if wrong == 'no_bias_correction' else (1 - BETAS[0] ** t, 1 - BETAS[1] ** t)
    denom = (v / bc2 + EPS).sqrt() if wrong == 'eps_inside_sqrt' else v.sqrt() / bc2 ** 0.5 + EPS
    return p - lr / bc1 * m / denom


@pytest.fixture(scope='module')
def small():
    return make_inputs(SMALL_ENDS)


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('max_norm', [100.0, 1.0, 0.0])
def test_inputs_expose_the_three_classic_adamw_mistakes(small, t, max_norm):
    """The bound means something only if a wrong formula breaks it: each of the three, evaluated exactly, must leave it on at least
    a tenth of the elements -- and the written-out right formula must sit far inside it (it is not the reference's code)."""
    norm = float(small['ss'].double().sqrt()) * GSCALE
    assert 1.0 < norm < 100.0                                            # max_norm = 100 is above the norm, 1 below it
    ref = reference('AdamW', small, t0=t - 1, max_norm=max_norm)
    bound = bounds('AdamW', small, ref)['p']
    assert float(((_adamw_formula(small, t, max_norm) - ref['p']).abs() / bound).max()) < 1e-3
    for wrong in ('no_bias_correction', 'coupled_decay', 'eps_inside_sqrt'):
        frac = float(((_adamw_formula(small, t, max_norm, wrong) - ref['p']).abs() > bound).double().mean())
        print(f't={t} max_norm={max_norm} {wrong}: {frac:.3f} of the elements outside the bound')
        assert frac >= 0.1, (wrong, frac)


# ------------------------------------------------------------------ parsing

def test_unsupported_optimizers_raise_by_name():
    from bonai_amd.optim import parse_optimizer
    with pytest.raises(NotImplementedError, match='Adagrad'):
        parse_optimizer(dict(type='Adagrad', lr=0.1))
    with pytest.raises(NotImplementedError, match='amsgrad'):
        parse_optimizer(dict(type='AdamW', lr=1e-3, amsgrad=True))
    with pytest.raises(NotImplementedError, match='dampening'):
        parse_optimizer(dict(type='SGD', lr=0.1, momentum=0.9, dampening=0.1))
    with pytest.raises(NotImplementedError, match='momentum'):
        parse_optimizer(dict(type='AdamW', lr=1e-3, momentum=0.9))
    assert parse_optimizer(dict(type='SGD', lr=0.1, momentum=0.9, dampening=0, nesterov=True)) == \
        ('SGD', dict(lr=0.1, momentum=0.9, weight_decay=0.0, nesterov=True))
    assert parse_optimizer(dict(type='AdamW', lr=1e-4, weight_decay=0.05, amsgrad=False)) == \
        ('AdamW', dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05))


def test_grad_clip_none_is_no_clip():
    from bonai_amd.optim import parse_grad_clip
    assert parse_grad_clip(dict(grad_clip=None)) is None and parse_grad_clip({}) is None and parse_grad_clip(None) is None
    assert parse_grad_clip(dict(grad_clip=dict(max_norm=35, norm_type=2))) == 35.0
    with pytest.raises(NotImplementedError, match='norm_type'):
        parse_grad_clip(dict(grad_clip=dict(max_norm=35, norm_type=1)))


@pytest.fixture(scope='module')
def headline():
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_scratch_2x_bonai.py'))
    return cfg, build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)


def test_norm_and_bias_rules_on_the_headline_model(headline):
    from bonai_amd.loft.backbone import FrozenStatBN
    from bonai_amd.optim import param_multipliers
    _, model = headline
    mults = param_multipliers(model, dict(norm_decay_mult=0., bias_decay_mult=0.5, bias_lr_mult=2.))
    names = [n for n, _ in model.named_parameters()]
    assert set(mults) == set(names)
    norm_params = {f'{mn}.{pn}' for mn, mod in model.named_modules() if isinstance(mod, FrozenStatBN) for pn, _ in mod.named_parameters(recurse=False)}
    assert 'backbone.bn1.weight' in norm_params and 'backbone.layer1.0.bn1.bias' in norm_params
    seen = set()
    for n in names:
        if n in norm_params:
            want = (1.0, 0.0)                        # a norm layer's bias is not a "bias" for bias_lr_mult
        elif n.endswith('.bias'):
            want = (2.0, 0.5)
        else:
            want = (1.0, 1.0)
        assert mults[n] == want, (n, mults[n], want)
        seen.add(want)
    assert seen == {(1.0, 0.0), (2.0, 0.5), (1.0, 1.0)}
    assert all(v == (1.0, 1.0) for v in param_multipliers(model, {}).values())
    # a norm bias falls under bias_decay_mult when norm_decay_mult is unset (the rule's "else")
    assert param_multipliers(model, dict(bias_decay_mult=0.))['backbone.bn1.bias'] == (1.0, 0.0)
    with pytest.raises(NotImplementedError, match='dwconv_decay_mult'):
        param_multipliers(model, dict(dwconv_decay_mult=0.))
    with pytest.raises(NotImplementedError, match='frobnicate'):
        param_multipliers(model, dict(frobnicate=1))


def test_custom_keys_longest_first_then_alphabetical(headline):
    from bonai_amd.optim import param_multipliers
    _, model = headline
    cfg = dict(norm_decay_mult=0., bias_lr_mult=2.,
               custom_keys={'backbone': dict(lr_mult=0.1), 'backbone.layer4': dict(lr_mult=0.5, decay_mult=0.25),
                            'bn1': dict(decay_mult=0.75), 'bn2': dict(decay_mult=0.125), 'rpn_head': dict(lr_mult=3.0)})
    mults = param_multipliers(model, cfg)
    assert mults['backbone.layer4.0.conv1.weight'] == (0.5, 0.25)        # the longer key wins over 'backbone'
    assert mults['backbone.layer4.0.bn1.weight'] == (0.5, 0.25)          # ... and over the norm rule and the shorter 'bn1'
    assert mults['backbone.layer1.0.conv1.weight'] == (0.1, 1.0)         # a custom key sets BOTH: the unset one is 1
    assert mults['backbone.layer1.0.bn1.weight'] == (0.1, 1.0)           # 'backbone' (8) before 'bn1' (3): no norm rule either
    assert mults['backbone.layer1.0.bn2.bias'] == (0.1, 1.0)
    rpn = [n for n in mults if n.startswith('rpn_head.')]
    assert rpn and all(mults[n] == (3.0, 1.0) for n in rpn)              # its biases too: bias_lr_mult does not apply after a key
    neck_bias = [n for n in mults if n.startswith('neck.') and n.endswith('.bias')]
    assert neck_bias and all(mults[n] == (2.0, 1.0) for n in neck_bias)
    # equal length: alphabetical -- a name containing both 'bn1' and 'bn2' cannot exist, so check the order on a synthetic module
    toy = torch.nn.Module()
    toy.ab_cd = torch.nn.Linear(2, 2)
    got = param_multipliers(toy, dict(custom_keys={'cd': dict(lr_mult=7.), 'ab': dict(lr_mult=5.), 'b_c': dict(lr_mult=9.)}))
    assert got['ab_cd.weight'] == (9.0, 1.0)
    got = param_multipliers(toy, dict(custom_keys={'cd': dict(lr_mult=7.), 'ab': dict(lr_mult=5.)}))
    assert got['ab_cd.weight'] == (5.0, 1.0)


def test_dcn_offset_lr_mult_reaches_conv_offset_only():
    from bonai_amd.loft.backbone import ModulatedDeformConvPack
    from bonai_amd.optim import param_multipliers
    toy = torch.nn.Module()
    toy.conv2 = ModulatedDeformConvPack(4, 4, 3, padding=1, bias=True)
    got = param_multipliers(toy, dict(dcn_offset_lr_mult=0.1, bias_lr_mult=2.))
    assert got == {'conv2.weight': (1.0, 1.0), 'conv2.bias': (2.0, 1.0), 'conv2.conv_offset.weight': (0.1, 1.0),
                   'conv2.conv_offset.bias': (0.1, 1.0)}


def _arena_slots(model):
    """FlatArena's layout (bonai_amd/engine.py) without allocating it: reverse registration order, slots padded to 8 floats."""
    slots, off = [], 0
    for n, p in reversed([(n, p) for n, p in model.named_parameters() if p.requires_grad]):
        length = (p.numel() + 7) // 8 * 8
        slots.append((n, off, length))
        off += length
    return slots, off


def test_segments_merge_and_cover_the_arena(headline):
    from bonai_amd.optim import arena_segments, build_spec
    _, model = headline
    slots, total = _arena_slots(model)
    spec = build_spec(dict(type='AdamW', lr=1e-4, weight_decay=0.05, paramwise_cfg=dict(norm_decay_mult=0., bias_decay_mult=0.)), model=model)
    assert spec.rule == 'AdamW' and spec.paramwise
    segs = arena_segments(spec, slots)
    ends = [e for e, _, _ in segs]
    assert ends[-1] == total and all(e % 8 == 0 for e in ends) and all(b > a for a, b in zip([0] + ends, ends))
    assert all((a[1], a[2]) != (b[1], b[2]) for a, b in zip(segs, segs[1:]))      # merged: neighbours differ
    assert 2 < len(segs) < len(slots) and len(segs) <= 512
    slot_of = {off: n for n, off, _ in slots}
    starts = [0] + ends[:-1]
    assert all(s in slot_of for s in starts)                                      # boundaries are slot boundaries
    for (n, off, length) in slots:                                                # every slot lies in a segment of its multipliers
        i = next(k for k, e in enumerate(ends) if off < e)
        assert off + length <= ends[i] and (segs[i][1], segs[i][2]) == spec.mult_of(n), n
    assert arena_segments(build_spec(dict(type='SGD', lr=0.1, momentum=0.9), model=model), slots) is None
    assert arena_segments(build_spec(dict(type='SGD', lr=0.1), paramwise_cfg={}, model=model), slots) is None


def test_train_tool_builds_the_trainer_from_the_config(headline):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train as train_tool
    finally:
        sys.path.pop(0)
    from bonai_amd.config import Config
    cfg0, model = headline
    kw = train_tool.optimizer_kwargs(cfg0, model)
    assert kw['optimizer'].rule == 'SGD' and kw['lr'] == 0.005 and kw['max_norm'] == 35.0
    assert kw['optimizer'].hyper == dict(lr=0.005, momentum=0.9, weight_decay=0.0001, nesterov=False) and not kw['optimizer'].paramwise
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_scratch_adamw_2x_bonai.py'))
    kw = train_tool.optimizer_kwargs(cfg, model)
    assert kw['optimizer'].rule == 'AdamW' and kw['optimizer'].paramwise and kw['lr'] == cfg.optimizer.lr
    assert kw['optimizer'].mult_of('backbone.bn1.weight') == (1.0, 0.0) and kw['optimizer'].mult_of('backbone.conv1.weight') == (1.0, 1.0)
    # --options optimizer.type=AdamW optimizer_config.grad_clip=None over the SGD config
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_scratch_2x_bonai.py'))
    options = ['optimizer.type=AdamW', 'optimizer_config.grad_clip=None']
    cfg.merge_from_dict(dict(train_tool.parse_option(o) for o in options))
    kw = train_tool.optimizer_kwargs(cfg, model, options)
    assert kw['optimizer'].rule == 'AdamW' and kw['max_norm'] is None
    assert kw['optimizer'].hyper == dict(lr=0.005, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0001)
    cfg.merge_from_dict({'optimizer.type': 'LAMB'})
    with pytest.raises(NotImplementedError, match='LAMB'):
        train_tool.optimizer_kwargs(cfg, model, ['optimizer.type=LAMB'])


def test_trainer_on_the_cpu_takes_the_spec_and_allocates_only_what_it_needs():
    """No device: the arena, the segment table and AdamW's second buffer are plain tensors (the kernels themselves need the GPU)."""
    from bonai_amd.engine import Trainer
    def toy():
        m = torch.nn.Module()
        m.fc = torch.nn.Linear(5, 3)
        m.norm = torch.nn.LayerNorm(6)
        return m
    plain = Trainer(toy(), lr=0.01)
    assert plain.optim is None and plain.seg_table is None and plain.exp_avg_sq is None and plain.opt_state is None and plain._plain_sgd
    sgd = Trainer(toy(), optimizer=dict(type='SGD', lr=0.02, momentum=0.8, weight_decay=0.0))
    assert sgd._plain_sgd and (sgd.lr, sgd.mu, sgd.wd) == (0.02, 0.8, 0.0) and sgd.exp_avg_sq is None
    assert not Trainer(toy(), optimizer=dict(type='SGD', lr=0.02, momentum=0.8, nesterov=True))._plain_sgd
    adam = Trainer(toy(), optimizer=dict(type='AdamW', lr=1e-3), paramwise_cfg=dict(norm_decay_mult=0.), max_norm=None)
    assert not adam._plain_sgd and adam.max_norm == 0.0 and adam.exp_avg_sq.shape == adam.arena.momentum.shape
    # arena order is reverse registration: norm.bias, norm.weight | fc.bias, fc.weight -> two segments
    assert adam.seg_table.segments == [(16, 1.0, 0.0), (16 + 8 + 16, 1.0, 1.0)]
    with pytest.raises(NotImplementedError, match='RMSprop'):
        Trainer(toy(), optimizer=dict(type='RMSprop', lr=0.1))
