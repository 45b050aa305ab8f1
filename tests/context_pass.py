"""The context pass, stated once: a call gives the bits of the FIRST call of a new context whatever the context has been through.

tests/test_gpu_context_state.py runs it over the table of tests/context_cases.py with legs of its own; the modules of the resident-map
entry points (tests/test_gpu_*_context.py) each declare one Pass - their calls, the sizes, and what runs between the compared calls - and
run the three legs below:

  after_legs  on ONE context: the call, the larger call(s), the call, the other entry points, the call;
  poisoned    option test_scratch_fill = v on a context that has run the prelude (every block filled at once), and on a new context
              before its first call (every block filled as it is allocated);
  timers_on   two rounds over all calls with the timers on (the second round takes its events from the pool).

Every compared result equals the reference: the outputs of the call as the first call of a brand-new context, computed once per process
and handed out read-only.  Equality is `same`: the same keys, dtypes and shapes, np.array_equal(..., equal_nan=True) on every key.

Test infrastructure; nothing in the product imports it."""
import dataclasses
import typing

import numpy as np
import pytest

from tests.context_cases import close_context, new_context

_first = {}  # (pass name, call name, size) -> outputs as the first call of a new context: made once, read-only


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU test collected without a GPU"
    return torch


def run(fn, torch, ctx):
    """fn(torch, ctx) - but a HIP error is a finding, not a mismatch: the session ends there instead of starting more work on a device
    that has just faulted"""
    from gmmloc_amd import api
    try:
        return fn(torch, ctx)
    except (api.GLError, RuntimeError) as e:
        if any(w in str(e) for w in ("HIP", "hip", "illegal memory access", "error -4")):
            pytest.exit("device error, nothing more is started: %s" % e, returncode=3)
        raise


def on_new_context(torch, fn, fill=None):
    ctx = new_context()
    try:
        if fill is not None:
            ctx.set_option("test_scratch_fill", fill)
        return run(fn, torch, ctx)
    finally:
        close_context(ctx)


def first_call(torch, key, fn):
    """the outputs of fn(torch, ctx) as the first call of a new context, made once per process under key = (pass, call, size); the
    arrays are the cache's own copies and read-only"""
    if key not in _first:
        out = {}
        for k, v in on_new_context(torch, fn).items():
            out[k] = np.array(v)
            out[k].setflags(write=False)
        _first[key] = out
    return _first[key]


def same(got, ref, label, leg):
    assert sorted(got) == sorted(ref), (label, leg, sorted(got), sorted(ref))
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (label, leg, k, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b, equal_nan=True):
            diff = ~((a == b) | ((a != a) & (b != b)))
            raise AssertionError("case %s, leg %s, output %s: %d of %d elements differ" % (label, leg, k, int(diff.sum()), a.size))


def at(fn, size):
    """fn(torch, ctx, size) as a callable of (torch, ctx)"""
    return lambda torch, ctx: fn(torch, ctx, size)


@dataclasses.dataclass
class Pass:
    name: str  # of the module: the first key of the reference cache
    calls: dict  # call name -> fn(torch, ctx, size)
    small: dict  # call name -> the size the reference is made with, and every compared call
    larger: typing.Callable  # call name -> the callables (torch, ctx) between the first and the second compared call
    others: tuple  # the callables between the second and the third
    prelude: tuple  # what the poisoned leg runs before it fills the blocks
    legs: tuple = ("after the larger call", "after mapping_pass_from_map")  # the labels of the second and third compared call

    def call(self, name):
        return at(self.calls[name], self.small[name])

    def first(self, torch, name):
        return first_call(torch, (self.name, name, self.small[name]), self.call(name))


def after_legs(torch, p, name):
    fn, ref = p.call(name), p.first(torch, name)
    ctx = new_context()
    try:
        same(run(fn, torch, ctx), ref, name, "first")
        for other in p.larger(name):
            run(other, torch, ctx)
        same(run(fn, torch, ctx), ref, name, p.legs[0])
        for other in p.others:
            run(other, torch, ctx)
        same(run(fn, torch, ctx), ref, name, p.legs[1])
    finally:
        close_context(ctx)


def poisoned(torch, p, name, v):
    fn, ref = p.call(name), p.first(torch, name)
    ctx = new_context()
    try:
        for pre in p.prelude:
            run(pre, torch, ctx)
        ctx.set_option("test_scratch_fill", v)  # every block the context holds, now
        same(run(fn, torch, ctx), ref, name, "blocks filled with 0x%02X" % v)
    finally:
        close_context(ctx)
    same(on_new_context(torch, fn, fill=v), ref, name, "new context, blocks filled with 0x%02X as they are allocated" % v)


def timers_on(torch, p):
    refs = {name: p.first(torch, name) for name in p.calls}
    ctx = new_context()
    try:
        ctx.timing(True)
        for _ in range(2):  # (the second round takes its events from the pool)
            for name in p.calls:
                same(run(p.call(name), torch, ctx), refs[name], name, "timers on")
    finally:
        close_context(ctx)
