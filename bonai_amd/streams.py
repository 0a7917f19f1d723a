"""Side-stream fork / join: the one vocabulary for running a chain of launches beside the current stream.

The caching allocator hands a freed block out again in the order of the stream it was allocated on, unless record_stream told
it about another stream that uses the block.  Two lifetime rules follow for what is passed to fork and join:
  * inputs, allocated on the forking stream and read on the side stream, need fork's record_stream only if they can be freed
    before the join.  What the caller keeps alive until after the join (a local, an attribute, a tensor autograd saved for a node
    that runs behind the join) crosses without one;
  * outputs, allocated on the side stream and consumed after the join, always need join's record_stream.
fork comes AFTER every lazily built table both sides read: a cached table queued for construction on one stream is not ordered
against the other (RPNHead._geometry builds the anchor tables in front of the proposal fork for that reason)."""
import contextlib

import torch

from . import kernels as K
from .debug import DBG


def owned(owner, attr):
    """The torch.cuda.Stream stored as ``owner.<attr>``, created on first use."""
    if getattr(owner, attr, None) is None:
        setattr(owner, attr, torch.cuda.Stream())
    return getattr(owner, attr)


def enabled(t):
    """Whether work on ``t`` may fork at all; a site with switches of its own adds them."""
    return t.is_cuda and torch.is_grad_enabled() and K.PROFILE is None and not DBG.no_side_stream


def fork(side, *reads):
    """``side`` waits for the current stream; ``reads`` are recorded on it (first rule)."""
    side.wait_stream(torch.cuda.current_stream())
    for t in reads:
        t.record_stream(side)


def join(side, *made, after=None):
    """The current stream waits for ``side`` -- or, joining a fork made in an earlier call, for the event ``after`` recorded on it
    then; ``made`` are recorded on the current stream (second rule)."""
    main = torch.cuda.current_stream()
    if after is None:
        main.wait_stream(side)
    else:
        main.wait_event(after)
    for t in made:
        t.record_stream(main)


def on(side):
    """Context: ``side`` is the current stream inside the block; None leaves the current stream alone."""
    return contextlib.nullcontext() if side is None else torch.cuda.stream(side)
