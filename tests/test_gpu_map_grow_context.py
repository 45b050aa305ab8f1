"""map_add, map_fuse and fuse_observations_from_map give the bits of the FIRST call of a new context whatever the context has been
through - the pass of tests/test_gpu_context_state.py for the module gmmloc_amd.map_grow, with that file's helpers: after larger calls
of themselves, after mapping_pass_from_map (which leaves gl_map_remove's marks in the scratch block the two calls use), with every
scratch block filled with 0x00 / 0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api
from tests import map_edit_scenes as ES
from tests import map_grow_scenes as GS
from tests.context_cases import BY_NAME, close_context, gt_sync, map_v1, new_context
from tests.test_gpu_context_state import on_new_context, run, torch  # noqa: F401 (torch: the module's fixture)
from tests.test_gpu_map_grow import device_add, device_fuse, device_pass, host_pass, ADD_KEYS, FUSE_KEYS

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _add_inputs(name):
    return GS.add_lists(ES.scene(name, name in ES.CLAMP), 2)


@functools.lru_cache(maxsize=None)
def _fuse_inputs(name):
    sc = ES.scene(name, name in ES.CLAMP)
    return (sc,) + GS.fuse_lists(sc, 1)


def _add(torch, ctx, name):
    m, ba, ref_kf, ls = _add_inputs(name)
    rows, res, _, _ = device_add(torch, ctx, m, ba, ref_kf, ls)
    return dict({k: np.asarray(rows[k]) for k in ADD_KEYS}, result=np.array(res))


def _fuse(torch, ctx, name):
    sc, kf, cand, best = _fuse_inputs(name)
    rows, res, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best)
    return dict({k: np.asarray(rows[k]) for k in FUSE_KEYS}, result=np.array(res))


@functools.lru_cache(maxsize=None)
def _geo():
    mean, cov = map_v1()
    return GS.geo_scene(mean, cov, gt_sync()["V1_01_easy"])


_cands = {}


def _composite(torch, ctx, _):
    """the composed pass of tests/test_gpu_map_grow.py on the resident arrays: three fuse_observations_from_map with refreshes between"""
    cam = api.Camera()
    if "c" not in _cands:  # (the candidate lists are inputs: made once, by the host route)
        c = new_context()
        try:
            _cands["c"] = host_pass(torch, c, _geo(), cam)[2]
        finally:
            close_context(c)
    sizes, out, steps = device_pass(torch, ctx, _geo(), cam, _cands["c"])
    return dict(out, sizes=np.array(sizes), steps=np.array([v for s in steps for v in s]))


CALLS = {"map_add": (_add, "small", "euroc"), "map_fuse": (_fuse, "small", "euroc"), "fuse_observations_from_map": (_composite, None, None)}
_first = {}


def first_call(torch, name):
    if name not in _first:
        fn, small, _ = CALLS[name]
        _first[name] = on_new_context(torch, lambda t, c: fn(t, c, small))
    return _first[name]


def same(got, ref, what):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, k)


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    """small, large, small on one context; then mapping_pass_from_map (large), then small again: each small equals the first call of a
    new context"""
    fn, small, large = CALLS[name]
    ref = first_call(torch, name)
    ctx = new_context()
    try:
        same(run(lambda t, c: fn(t, c, small), torch, ctx), ref, (name, "first"))
        if large is not None:
            run(lambda t, c: fn(t, c, large), torch, ctx)
        else:
            run(lambda t, c: _add(t, c, "euroc"), torch, ctx)  # (the composite has one size: the larger calls are its parts')
            run(lambda t, c: _fuse(t, c, "euroc"), torch, ctx)
        same(run(lambda t, c: fn(t, c, small), torch, ctx), ref, (name, "after the larger call"))
        run(BY_NAME["mapping_pass_from_map"].large, torch, ctx)
        same(run(lambda t, c: fn(t, c, small), torch, ctx), ref, (name, "after mapping_pass_from_map"))
    finally:
        close_context(ctx)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    fn, small, _ = CALLS[name]
    ref = first_call(torch, name)
    ctx = new_context()
    try:
        run(lambda t, c: _add(t, c, "euroc"), torch, ctx)
        run(lambda t, c: _fuse(t, c, "euroc"), torch, ctx)
        ctx.set_option("test_scratch_fill", v)  # every block the context holds, now
        same(run(lambda t, c: fn(t, c, small), torch, ctx), ref, (name, "blocks filled with 0x%02X" % v))
    finally:
        close_context(ctx)
    same(on_new_context(torch, lambda t, c: fn(t, c, small), fill=v), ref, (name, "new context, blocks filled with 0x%02X as they are allocated" % v))


def test_timers_on(torch):
    refs = {name: first_call(torch, name) for name in CALLS}
    ctx = new_context()
    try:
        ctx.timing(True)
        for _ in range(2):
            for name, (fn, small, _) in CALLS.items():
                same(run(lambda t, c: fn(t, c, small), torch, ctx), refs[name], (name, "timers on"))
    finally:
        close_context(ctx)
