"""bonai_amd.streams: the side-stream fork / join vocabulary of the RPN head, the RoI head, HRNet's branches and the
residual blocks' weight gradients."""
import pytest
import torch

from bonai_amd import kernels as K
from bonai_amd import streams
from bonai_amd.debug import DBG

pytestmark = pytest.mark.gpu


class _Owner:
    pass


def test_owned_creates_the_stream_once():
    o = _Owner()
    s = streams.owned(o, '_side_stream')
    assert isinstance(s, torch.cuda.Stream) and o._side_stream is s
    assert streams.owned(o, '_side_stream') is s
    assert streams.owned(o, '_loss_stream') is not s and o._side_stream is s


def test_on_switches_the_current_stream_and_restores_it():
    main = torch.cuda.current_stream()
    with streams.on(None):
        assert torch.cuda.current_stream() == main
    side = torch.cuda.Stream()
    with streams.on(side):
        assert torch.cuda.current_stream() == side
        with streams.on(None):
            assert torch.cuda.current_stream() == side
    assert torch.cuda.current_stream() == main


def test_fork_join_round_trip_equals_the_single_stream_computation():
    """main fills x, the side stream computes y from x behind fork, main reads y behind join; twice in a row on the same owned
    stream, as the RoI head forks its bbox and its mask branch."""
    def work(x):
        for _ in range(8):
            x = (x * 1.0009765625 + 0.5).sin()
        return x

    o = _Owner()
    gen = torch.Generator(device='cuda').manual_seed(0)
    for n in (4096, 5003):
        x = torch.randn(n, device='cuda', generator=gen) * 3
        side = streams.owned(o, '_side_stream')
        streams.fork(side, x)
        with streams.on(side):
            y = work(x)
        streams.join(side, y)
        got = y.sum() + y[::7].abs().sum()
        want_y = work(x)
        assert torch.equal(y, want_y)
        assert torch.equal(got, want_y.sum() + want_y[::7].abs().sum())
    assert o._side_stream is side


def test_join_after_an_event_of_an_earlier_fork():
    side = torch.cuda.Stream()
    x = torch.arange(3000, device='cuda', dtype=torch.float32)
    streams.fork(side, x)
    with streams.on(side):
        y = x * 2 + 1
        done = torch.cuda.Event()
        done.record(side)
    streams.join(side, y, after=done)
    assert torch.equal(y + 0, torch.arange(3000, device='cuda', dtype=torch.float32) * 2 + 1)


def test_enabled_is_the_shared_predicate():
    t = torch.zeros(4, device='cuda')
    assert streams.enabled(t)
    assert not streams.enabled(t.cpu())
    with torch.no_grad():
        assert not streams.enabled(t)
    saved, K.PROFILE = K.PROFILE, []
    try:
        assert not streams.enabled(t)
    finally:
        K.PROFILE = saved
    with DBG.override(no_side_stream=True):
        assert not streams.enabled(t)
    assert streams.enabled(t)
