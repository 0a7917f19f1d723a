"""CPU: the decision table of the autograd layer's parameter-gradient deposit (bonai_amd/nn.py).

A backward node that holds a packed weight gradient (and maybe a bias or BN gradient) either deposits it in the trainer's flat
arena -- through the unpack queue, or with a direct loft_fold_unpack_bwd(out=...) launch -- or hands it back to autograd.  The
backward bodies are driven here on CPU tensors with a fake queue and a fake sink on nn.UNPACK_Q / nn.GRAD_SINK and recorders in
place of the kernels: what is asserted is the exact list of queue records, which parameters were marked as sunk, every
parameter's final use count, when the sink fired and which gradients came back to autograd.  A parameter's "slot" is its .grad
(contiguous fp32, as the trainer's arena views are); a parameter "without a slot" has a non-contiguous .grad."""
from types import SimpleNamespace as NS

import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import nn as F2
from bonai_amd.debug import DBG


class _Queue:
    """Stands in for kernels.UnpackQueue: records add() and runs the callbacks at flush()."""

    def __init__(self):
        self.calls, self.done = [], []

    def add(self, dwp, db, w, bn, eps, slots, on_done=(), flat_chw=None, nsplit=1, params=()):
        self.calls.append(NS(dwp=dwp, db=db, w=w, bn=bn, eps=eps, slots=tuple(slots), flat_chw=flat_chw, nsplit=nsplit,
                             params=list(params)))
        self.done.extend(on_done)

    def flush(self):
        done, self.done = self.done, []
        for f in done:
            f()


def _same(a, b):
    """The same view of the same memory (or both None)?"""
    if a is None or b is None:
        return a is None and b is None
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _ids(ps):
    return [id(p) for p in ps]


class _Rig:
    def __init__(self, mp, queue, **switches):
        self.q = _Queue() if queue else None
        self.fired = []            # parameters the sink was told about, in order
        self.wgrads = []           # (slots_ok, dwp, db) of every weight-gradient launch
        self.direct = []           # fold_unpack_bwd(out=...) calls
        self.unpacked = []         # fold_unpack_bwd(...) calls whose results go back to autograd
        self.params = []
        mp.setattr(F2, 'UNPACK_Q', self.q)
        mp.setattr(F2, 'GRAD_SINK', self.fired.append)
        mp.setattr(K, 'conv2d_wgrad', self._wgrad)
        mp.setattr(K, 'fold_unpack_bwd', self._unpack)
        mp.setattr(K, 'narrow_head_bwd', self._narrow)
        for k, v in switches.items():
            mp.setattr(DBG, k, v)

    def param(self, *shape, slot=True, uses=1):
        p = torch.nn.Parameter(torch.randn(*shape))
        if slot:
            p.grad = torch.zeros(*shape)
        else:                       # the right shape and dtype, but not contiguous: no arena slot
            p.grad = torch.zeros(*shape[:-1], 2 * shape[-1])[..., ::2]
            assert not p.grad.is_contiguous() and p.grad.shape == p.shape
        p._loft_pending = uses      # as the forward passes count them
        self.params.append(p)
        return p

    # ---- the kernels' stand-ins
    def _wgrad(self, g, x, R, S, stride=1, pad=0, groups=1, splits=0, with_bias=False, slots_ok=False):
        Cout, Cin = g.shape[1] // groups, x.shape[1] // groups
        # two split-K slots when the caller accepts them: the record must then carry nsplit == 2
        dwp = torch.randn(*((groups, 2) if slots_ok else (groups,)), R * S, Cout, Cin)
        db = torch.randn(groups, Cout) if with_bias else None
        self.wgrads.append(NS(slots_ok=bool(slots_ok), dwp=dwp, db=db))
        return (dwp, db) if with_bias else dwp

    def _unpack(self, dwp, db, w, bn=None, eps=1e-5, need_dw=True, out=None):
        rec = NS(dwp=dwp, db=db, w=w, bn=bn, eps=eps, need_dw=need_dw, out=out)
        if out is not None:
            self.direct.append(rec)
            return out
        self.unpacked.append(rec)
        vec = (lambda: torch.zeros(w.shape[0])) if bn is not None else (lambda: None)
        return (torch.zeros_like(w) if need_dw else None), vec(), vec()

    def _narrow(self, g, x, w, relu_in=False, need_gx=True, need_dw=True, need_db=True):
        self.narrow = NS(dw=torch.randn(w.shape[0], w.shape[1]) if need_dw else None,
                         db=torch.randn(w.shape[0]) if need_db else None)
        return None, self.narrow.dw, self.narrow.db

    # ---- what happened
    def sunk(self):
        return [id(p) for p in self.params if getattr(p, '_loft_sunk', False)]

    def pending(self):
        return [p._loft_pending for p in self.params]

    def flush(self):
        if self.q is not None:
            assert self.fired == [], 'the sink fired before the queue served the record'
            self.q.flush()

    def check_add(self, c, dwp, db, w, bn, eps, slots, nsplit, flat_chw, params):
        assert _same(c.dwp, dwp) and _same(c.db, db) and c.w is w
        assert (c.bn is None) == (bn is None) and (bn is None or all(a is b for a, b in zip(c.bn, bn))) and c.eps == eps
        assert len(c.slots) == 3 and all(a is b for a, b in zip(c.slots, slots))
        assert c.nsplit == nsplit and c.flat_chw == flat_chw and _ids(c.params) == _ids(params)


@pytest.fixture()
def rig(monkeypatch):
    return lambda queue, **sw: _Rig(monkeypatch, queue, **sw)


def _nonnull(grads):
    return [g is not None for g in grads]


# ------------------------------------------------------------------ _ConvFn

def _conv_bwd(tensors, G, has_b, bn_stats, needs_params, cin, cout):
    meta = (1, 1, False, G, False, has_b, bn_stats, False, False, None)
    x, g = torch.randn(2, G * cin, 5, 5), torch.randn(2, G * cout, 5, 5)
    ctx = NS(meta=meta, saved_tensors=(x, None, None) + tuple(tensors), params=tuple(tensors), in_hw=(5, 5), has_res=False,
             needs_input_grad=(False, False, False) + tuple(needs_params))
    out = F2._ConvFn.backward(ctx, g)
    assert out[:3] == (None, None, None)
    return out[3:]


def _conv_bn(r, gamma_slot=True, uses=1):
    w, gamma, beta = r.param(8, 4, 3, 3, uses=uses), r.param(8, slot=gamma_slot, uses=uses), r.param(8, uses=uses)
    stats = (torch.zeros(8), torch.ones(8), 1e-3)
    run = lambda: _conv_bwd((w, None, gamma, beta), 1, False, stats, (True, False, True, True), 4, 8)
    return w, gamma, beta, stats, run


def test_conv_bn_queue(rig):
    r = rig(True)
    w, gamma, beta, stats, run = _conv_bn(r)
    grads = run()
    (wg,) = r.wgrads
    assert wg.slots_ok and len(r.q.calls) == 1 and not r.direct and not r.unpacked
    r.check_add(r.q.calls[0], wg.dwp[0], wg.db[0], w, (gamma, beta, stats[0], stats[1]), 1e-3, (w.grad, gamma.grad, beta.grad),
                2, None, [w, gamma, beta])
    assert _nonnull(grads) == [False, False, False, False]
    assert r.sunk() == _ids([w, gamma, beta]) and r.pending() == [1, 1, 1]
    r.flush()
    assert _ids(r.fired) == _ids([w, gamma, beta]) and r.pending() == [0, 0, 0]


def test_conv_bn_direct(rig):
    r = rig(False)
    w, gamma, beta, stats, run = _conv_bn(r)
    grads = run()
    (wg,) = r.wgrads
    (d,) = r.direct
    assert not wg.slots_ok and not r.unpacked
    assert _same(d.dwp, wg.dwp[0]) and _same(d.db, wg.db[0]) and d.w is w and d.eps == 1e-3
    assert all(a is b for a, b in zip(d.bn, (gamma, beta, stats[0], stats[1])))
    assert all(a is b for a, b in zip(d.out, (w.grad, gamma.grad, beta.grad)))
    assert _nonnull(grads) == [False, False, False, False]
    assert r.sunk() == _ids([w, gamma, beta]) and r.pending() == [0, 0, 0]
    assert _ids(r.fired) == _ids([w, gamma, beta])


@pytest.mark.parametrize('queue', [True, False])
def test_conv_bn_missing_slot_goes_to_autograd(rig, queue):
    r = rig(queue)
    w, gamma, beta, stats, run = _conv_bn(r, gamma_slot=False)
    grads = run()
    (wg,) = r.wgrads
    (u,) = r.unpacked
    assert not wg.slots_ok and not r.direct and (r.q is None or not r.q.calls)
    assert _same(u.dwp, wg.dwp[0]) and _same(u.db, wg.db[0]) and u.w is w and u.eps == 1e-3 and u.need_dw
    assert _nonnull(grads) == [True, False, True, True]
    r.flush()
    assert r.sunk() == [] and r.pending() == [0, 0, 0] and r.fired == []       # (handed to autograd: the uses are taken back)


@pytest.mark.parametrize('queue', [True, False])
def test_sink_fires_once_after_the_last_use(rig, queue):
    r = rig(queue)
    w, gamma, beta, stats, run = _conv_bn(r, uses=2)
    run()
    r.flush()
    assert r.fired == [] and r.pending() == [1, 1, 1]
    run()
    r.flush()
    assert _ids(r.fired) == _ids([w, gamma, beta]) and r.pending() == [0, 0, 0]


def _grouped(r, w1_slot=True):
    """Two groups with conv biases; the second bias has no slot."""
    w0, b0, w1, b1 = r.param(8, 4, 3, 3), r.param(8), r.param(8, 4, 3, 3, slot=w1_slot), r.param(8, slot=False)
    return w0, b0, w1, b1, (lambda: _conv_bwd((w0, b0, w1, b1), 2, True, None, (True, True, True, True), 4, 8))


def test_grouped_conv_queue_slotless_bias_alone_goes_to_autograd(rig):
    r = rig(True)
    w0, b0, w1, b1, run = _grouped(r)
    grads = run()
    (wg,) = r.wgrads
    assert wg.slots_ok and len(r.q.calls) == 2 and not r.direct and not r.unpacked        # (the biases are not in the predicate)
    r.check_add(r.q.calls[0], wg.dwp[0], wg.db[0], w0, None, 1e-5, (w0.grad, None, b0.grad), 2, None, [w0, b0])
    r.check_add(r.q.calls[1], wg.dwp[1], wg.db[1], w1, None, 1e-5, (w1.grad, None, None), 2, None, [w1])
    assert _nonnull(grads) == [False, False, False, True] and _same(grads[3], wg.db[1][:8])
    assert r.sunk() == _ids([w0, b0, w1])
    r.flush()
    assert _ids(r.fired) == _ids([w0, b0, w1]) and r.pending() == [0, 0, 0, 0]


def test_grouped_conv_direct_sinks_the_weights_only(rig):
    r = rig(False)
    w0, b0, w1, b1, run = _grouped(r)
    grads = run()
    (wg,) = r.wgrads
    assert not wg.slots_ok and len(r.direct) == 2 and not r.unpacked
    for i, (d, w) in enumerate(zip(r.direct, (w0, w1))):
        assert _same(d.dwp, wg.dwp[i]) and _same(d.db, wg.db[i]) and d.w is w and d.bn is None and d.eps == 1e-5
        assert d.out[0] is w.grad and d.out[1] is None and d.out[2] is None
    assert _nonnull(grads) == [False, True, False, True]
    assert _same(grads[1], wg.db[0][:8]) and _same(grads[3], wg.db[1][:8])
    assert r.sunk() == _ids([w0, w1]) and _ids(r.fired) == _ids([w0, w1]) and r.pending() == [0, 0, 0, 0]


def test_grouped_conv_queue_group_without_weight_slot_goes_to_autograd(rig):
    r = rig(True)
    w0, b0, w1, b1, run = _grouped(r, w1_slot=False)
    grads = run()
    (wg,) = r.wgrads
    (u,) = r.unpacked
    assert not wg.slots_ok and len(r.q.calls) == 1 and not r.direct        # atomically combined form: nsplit 1
    r.check_add(r.q.calls[0], wg.dwp[0], wg.db[0], w0, None, 1e-5, (w0.grad, None, b0.grad), 1, None, [w0, b0])
    assert _same(u.dwp, wg.dwp[1]) and _same(u.db, wg.db[1]) and u.w is w1 and u.bn is None and u.need_dw
    assert _nonnull(grads) == [False, False, True, True] and _same(grads[3], wg.db[1][:8])
    assert r.sunk() == _ids([w0, b0])
    r.flush()
    assert _ids(r.fired) == _ids([w0, b0]) and r.pending() == [0, 0, 0, 0]


# ------------------------------------------------------------------ _LinearFn with flat_chw

def _linear(r, b_slot=True):
    O, C, H, W = 6, 4, 2, 2
    w, b = r.param(O, C * H * W), r.param(O, slot=b_slot)
    x4 = torch.randn(3, C * H * W, 1, 1).to(K.L.act16())
    ctx = NS(cfg=(False, False, (C, H, W), (3, C, H, W)), saved_tensors=(x4, None, None, w), params=(w, b),
             needs_input_grad=(False, True, True, False, False, False))
    return w, b, (lambda: F2._LinearFn.backward(ctx, torch.randn(3, O)))


def test_linear_flat_chw_queue(rig):
    r = rig(True)
    w, b, run = _linear(r)
    grads = run()
    (wg,) = r.wgrads
    assert wg.slots_ok and len(r.q.calls) == 1 and not r.direct and not r.unpacked
    r.check_add(r.q.calls[0], wg.dwp[0, :, 0], wg.db[0], w, None, 1e-5, (w.grad, None, b.grad), 2, (4, 2, 2), [w, b])
    assert _nonnull(grads) == [False] * 6 and r.sunk() == _ids([w, b])
    r.flush()
    assert _ids(r.fired) == _ids([w, b]) and r.pending() == [0, 0]


@pytest.mark.parametrize('queue,b_slot', [(False, True), (True, False)])
def test_linear_flat_chw_without_queue_or_slot_goes_to_autograd(rig, queue, b_slot):
    r = rig(queue)
    w, b, run = _linear(r, b_slot=b_slot)
    grads = run()
    (wg,) = r.wgrads
    assert not wg.slots_ok and not r.direct and not r.unpacked and (r.q is None or not r.q.calls)
    assert _nonnull(grads) == [False, True, True, False, False, False]
    want = wg.dwp[0, 0, :6, :16].reshape(6, 4, 4).permute(0, 2, 1).reshape(6, 16)     # (h, w, c) columns back to (c, h, w)
    assert torch.equal(grads[1], want) and _same(grads[2], wg.db[0, :6])
    r.flush()
    assert r.sunk() == [] and r.fired == [] and r.pending() == [1, 1]


# ------------------------------------------------------------------ _NarrowHeadFn with two leaves

def _narrow(r, bb_slot=True):
    wa, ba, wb, bb = r.param(2, 8), r.param(2), r.param(4, 8), r.param(4, slot=bb_slot)
    w = torch.cat([wa, wb]).detach().view(6, 8, 1, 1)
    ctx = NS(saved_tensors=(torch.randn(2, 8, 3, 3), w), sp=(1, 0), has_b=True, input_relu=False,
             leaves=[(wa, ba, 0, 2), (wb, bb, 2, 6)], needs_input_grad=(False, True, True) + (False,) * 6)
    return wa, ba, wb, bb, (lambda: F2._NarrowHeadFn.backward(ctx, torch.randn(2, 8, 3, 3)))


def test_narrow_head_leaves_queue(rig):
    r = rig(True)
    wa, ba, wb, bb, run = _narrow(r)
    grads = run()
    dw, db = r.narrow.dw, r.narrow.db
    assert len(r.q.calls) == 2 and not r.direct and not r.unpacked and not r.wgrads
    r.check_add(r.q.calls[0], dw[0:2], db[0:2], wa, None, 1e-5, (wa.grad, None, ba.grad), 1, None, [wa, ba])
    r.check_add(r.q.calls[1], dw[2:6], db[2:6], wb, None, 1e-5, (wb.grad, None, bb.grad), 1, None, [wb, bb])
    assert _nonnull(grads) == [False] * 9 and r.sunk() == _ids([wa, ba, wb, bb])
    r.flush()
    assert _ids(r.fired) == _ids([wa, ba, wb, bb]) and r.pending() == [0, 0, 0, 0]


@pytest.mark.parametrize('queue,bb_slot,switches', [(False, True, {}), (True, False, {}), (True, True, {'no_leaf_sink': True})])
def test_narrow_head_leaves_all_or_nothing(rig, queue, bb_slot, switches):
    """No queue, one leaf without a slot, or DBG.no_leaf_sink: nothing is marked, everything goes to autograd and the uses the
    forward counted are taken back."""
    r = rig(queue, **switches)
    wa, ba, wb, bb, run = _narrow(r, bb_slot=bb_slot)
    grads = run()
    assert not r.direct and not r.unpacked and (r.q is None or not r.q.calls)
    assert _nonnull(grads) == [False, True, True] + [False] * 6
    assert grads[1].shape == (6, 8, 1, 1) and _same(grads[1].view(6, 8), r.narrow.dw) and grads[2] is r.narrow.db
    r.flush()
    assert r.sunk() == [] and r.fired == [] and r.pending() == [0, 0, 0, 0]


# ------------------------------------------------------------------ one conv+bn of a residual block

def _rb(r, needs, beta_slot=True, w_slot=True):
    w, gamma, beta = r.param(8, 4, 3, 3, slot=w_slot), r.param(8), r.param(8, slot=beta_slot)
    bn = NS(weight=gamma, bias=beta, running_mean=torch.zeros(8), running_var=torch.ones(8), eps=1e-3)
    g, x = torch.randn(2, 8, 5, 5), torch.randn(2, 4, 5, 5)
    return w, bn, (lambda: F2._rb_param_grads(g, x, w, bn, 3, 1, 1, needs))


def _bnt(bn):
    return bn.weight, bn.bias, bn.running_mean, bn.running_var


def test_res_block_conv_queue(rig):
    r = rig(True)
    w, bn, run = _rb(r, (True, True, True))
    grads = run()
    (wg,) = r.wgrads
    assert wg.slots_ok and len(r.q.calls) == 1 and not r.direct and not r.unpacked
    r.check_add(r.q.calls[0], wg.dwp[0], wg.db[0], w, _bnt(bn), 1e-3, (w.grad, bn.weight.grad, bn.bias.grad), 2, None,
                [w, bn.weight, bn.bias])
    assert _nonnull(grads) == [False, False, False] and r.sunk() == _ids([w, bn.weight, bn.bias])
    r.flush()
    assert _ids(r.fired) == _ids([w, bn.weight, bn.bias]) and r.pending() == [0, 0, 0]


def test_res_block_conv_direct(rig):
    r = rig(False)
    w, bn, run = _rb(r, (True, True, True))
    grads = run()
    (wg,) = r.wgrads
    (d,) = r.direct
    assert not wg.slots_ok and not r.unpacked
    assert _same(d.dwp, wg.dwp[0]) and _same(d.db, wg.db[0]) and d.w is w and d.eps == 1e-3
    assert all(a is b for a, b in zip(d.bn, _bnt(bn))) and all(a is b for a, b in zip(d.out, (w.grad, bn.weight.grad, bn.bias.grad)))
    assert _nonnull(grads) == [False, False, False]
    assert r.sunk() == _ids([w, bn.weight, bn.bias]) and _ids(r.fired) == _ids([w, bn.weight, bn.bias]) and r.pending() == [0, 0, 0]


@pytest.mark.parametrize('queue', [True, False])
def test_res_block_conv_missing_slot_goes_to_autograd(rig, queue):
    r = rig(queue)
    w, bn, run = _rb(r, (True, True, True), beta_slot=False)
    grads = run()
    (wg,) = r.wgrads
    (u,) = r.unpacked
    assert not wg.slots_ok and not r.direct and (r.q is None or not r.q.calls)
    assert _same(u.dwp, wg.dwp[0]) and _same(u.db, wg.db[0]) and u.w is w and u.eps == 1e-3 and u.need_dw
    assert _nonnull(grads) == [True, True, True]
    r.flush()
    assert r.sunk() == [] and r.fired == [] and r.pending() == [1, 1, 1]


@pytest.mark.parametrize('queue,w_slot', [(True, True), (False, True), (True, False)])
def test_res_block_conv_weight_only_never_sinks(rig, queue, w_slot):
    """Only the weight gradient is asked for (frozen BN affine): the block's deposit needs all three, so autograd gets dW."""
    r = rig(queue)
    w, bn, run = _rb(r, (True, False, False), w_slot=w_slot)
    grads = run()
    (wg,) = r.wgrads
    (u,) = r.unpacked
    assert not wg.slots_ok and not r.direct and (r.q is None or not r.q.calls) and u.need_dw
    assert _nonnull(grads) == [True, False, False]
    r.flush()
    assert r.sunk() == [] and r.fired == [] and r.pending() == [1, 1, 1]


def test_res_block_conv_nothing_asked_launches_nothing(rig):
    r = rig(True)
    w, bn, run = _rb(r, (False, False, False))
    assert run() == (None, None, None) and not r.wgrads and not r.q.calls and not r.unpacked
