"""map_add, map_fuse and fuse_observations_from_map give the bits of the FIRST call of a new context whatever the context has been
through - the pass of tests/context_pass.py for the module gmmloc_amd.map_grow: after larger calls
of themselves, after mapping_pass_from_map (which leaves gl_map_remove's marks in the scratch block the two calls use), with every
scratch block filled with 0x00 / 0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api
from tests import map_edit_scenes as ES
from tests import map_grow_scenes as GS
from tests.context_cases import BY_NAME, close_context, gt_sync, map_v1, new_context
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)
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


CALLS = {"map_add": _add, "map_fuse": _fuse, "fuse_observations_from_map": _composite}
GROW = (at(_add, "euroc"), at(_fuse, "euroc"))
# (the composite has one size: the larger calls are its parts')
PASS = Pass("map_grow", CALLS, small={"map_add": "small", "map_fuse": "small", "fuse_observations_from_map": None},
            larger=lambda name: GROW if name == "fuse_observations_from_map" else (at(CALLS[name], "euroc"),),
            others=(BY_NAME["mapping_pass_from_map"].large,), prelude=GROW)


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    """small, large, small on one context; then mapping_pass_from_map (large), then small again: each small equals the first call of a
    new context"""
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
