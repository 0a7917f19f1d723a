"""CPU: nn.installed(), the one place that sets and restores the trainer's hand-over globals (bonai_amd/nn.py's PREPACK,
HUB_ENABLED, HUB, JOIN, GRAD_SINK, UNPACK_Q, WGRAD_STREAM, PACK_TRACE and kernels.WEIGHT_PLANES).  The helper alone, with
sentinel objects: what is installed inside a scope, what is back after it -- after a normal exit, after a raise, and for two
nested scopes (the hipGraph capture runs inside a trainer step) -- that an unknown name changes nothing, and which module each
name lives in."""
import pytest

from bonai_amd import kernels as K
from bonai_amd import nn as F2

NAMES = ('PREPACK', 'HUB_ENABLED', 'HUB', 'JOIN', 'GRAD_SINK', 'UNPACK_Q', 'WGRAD_STREAM', 'PACK_TRACE', 'WEIGHT_PLANES')


def _home(name):
    return K if name == 'WEIGHT_PLANES' else F2


def _now():
    return {n: getattr(_home(n), n) for n in NAMES}


def _same(a, b):
    return a.keys() == b.keys() and all(a[n] is b[n] for n in a)


def test_the_helper_knows_exactly_the_written_out_names():
    assert tuple(F2._HANDOVER) == NAMES


def test_values_are_installed_inside_and_restored_after_a_normal_exit():
    before = _now()
    new = {n: object() for n in NAMES}
    with F2.installed(**new):
        assert _same(_now(), new)
    assert _same(_now(), before)


def test_values_are_restored_after_a_raise():
    before = _now()
    new = {n: object() for n in NAMES}
    with pytest.raises(ZeroDivisionError):
        with F2.installed(**new):
            assert _same(_now(), new)
            1 / 0
    assert _same(_now(), before)


def test_a_scope_touches_only_the_names_it_was_given():
    before = _now()
    q = object()
    with F2.installed(UNPACK_Q=q):
        assert _same(_now(), dict(before, UNPACK_Q=q))
    assert _same(_now(), before)


def test_nested_scopes_restore_the_outer_values_not_none():
    before = _now()
    outer = {n: object() for n in NAMES}
    inner = {n: object() for n in ('PREPACK', 'HUB_ENABLED', 'GRAD_SINK', 'UNPACK_Q', 'WGRAD_STREAM', 'PACK_TRACE', 'WEIGHT_PLANES')}
    with F2.installed(**outer):
        with F2.installed(**inner):
            assert _same(_now(), dict(outer, **inner))
        assert _same(_now(), outer)                       # the outer scope's objects, not None
        with pytest.raises(ZeroDivisionError):
            with F2.installed(**inner):
                1 / 0
        assert _same(_now(), outer)
    assert _same(_now(), before)


def test_the_same_name_twice_in_a_row_unwinds_in_reverse_order():
    before = _now()
    a, b = {}, {}
    with F2.installed(JOIN=a):
        with F2.installed(JOIN=b):
            assert F2.JOIN is b
        assert F2.JOIN is a
    assert _same(_now(), before)


@pytest.mark.parametrize('bad', [dict(PAIR_G={}), dict(JOIN={}, NO_SUCH=1), dict(GRAD_SINK=print, _USES={}), dict(K=None)])
def test_an_unknown_name_raises_and_changes_nothing(bad):
    before = _now()
    pair_g, uses = F2.PAIR_G, F2._USES
    entered = []
    with pytest.raises(TypeError, match='hand-over'):
        with F2.installed(**bad):
            entered.append(1)
    assert not entered
    assert _same(_now(), before)
    assert F2.PAIR_G is pair_g and F2._USES is uses and F2.K is K and not hasattr(F2, 'NO_SUCH')


def test_weight_planes_lands_on_kernels_the_rest_on_nn():
    new = {n: object() for n in NAMES}
    with F2.installed(**new):
        assert K.WEIGHT_PLANES is new['WEIGHT_PLANES']
        assert not hasattr(F2, 'WEIGHT_PLANES')
        for n in NAMES[:-1]:
            assert getattr(F2, n) is new[n]
            assert getattr(K, n, None) is not new[n]
    assert not hasattr(F2, 'WEIGHT_PLANES')
