"""The five calls of gmmloc_amd.covis and search_in_neighbors_from_map give the bits of the FIRST call of a new context whatever the
context has been through - the pass of tests/test_gpu_map_stats_context.py for this module, with that file's pattern: on a cold
context, after larger calls of themselves, after the other entry points of the resident map (which leave their marks in the two
scratch blocks these calls use), with every scratch block filled with 0x00 / 0xFF, and with the timers on."""
import copy
import functools

import numpy as np
import pytest

from gmmloc_amd import api, covis
from tests import covis_cases as CC
from tests import covis_dev as D
from tests import map_grow_scenes as GS
from tests.context_cases import BY_NAME, close_context, gt_sync, map_v1, new_context
from tests.test_gpu_context_state import on_new_context, run, torch  # noqa: F401 (torch: the module's fixture)
from tests.test_gpu_covis import _host, _scene, cand_inputs
from tests.test_gpu_map_grow_context import _add, _fuse, same

pytestmark = pytest.mark.gpu

WIDE = 4200  # more key-frames than the counters' LDS form takes: they live in the context's scratch


def _graph(torch, ctx, size):
    """updates, removals, lists and targets on a random map (small) / the same with twice the edits (large)"""
    m = CC.random_map(21)
    dg = D.DevGraph(torch, CC.graph(CC.R_NKF, CC.R_NKF, {}))
    mdev = D.dev_map(torch, m)
    out = {}
    for i, step in enumerate(CC.random_steps(121, 40 if size == "small" else 80)):
        if step[0] == "update":
            out.update({"u%d_%s" % (i, k): v for k, v in D.d_update(torch, ctx, mdev, dg, step[1], 8).items()})
        elif step[0] == "remove":
            out["r%d" % i] = D.d_remove(torch, ctx, dg, CC.R_NKF, step[1], step[2])
    kf = int(np.argmax(dg.host()["cov_nord"]))
    out.update({"t_" + k: v for k, v in D.d_targets(torch, ctx, dg, CC.R_NKF, m["kf_valid"], kf, 10, 5, 60).items()})
    out.update({"b_" + k: v for k, v in D.d_best(torch, ctx, dg, CC.R_NKF, list(range(CC.R_NKF)), 3, 4).items()})
    out.update(dg.host())
    return out


def _graph_wide(torch, ctx, size):
    """WIDE key-frame rows: the counters and the ranked row go through the scratch; small: three observers, large: forty"""
    n = 3 if size == "small" else 40
    m = CC.shared_map({(0, k): 10 + k for k in range(1, n + 1)}, nkf=WIDE, nfk=1300)
    dg = D.DevGraph(torch, CC.graph(WIDE, 4, {1: ([(2, 30)], 1)}) if size == "small" else CC.graph(WIDE, 48, {}))
    out = D.d_update(torch, ctx, D.dev_map(torch, m), dg, 0, 8)
    g = dg.host()
    return dict(out, **{k: g[k][:64] for k in g})


def _candidates(torch, ctx, size):
    npos = 257 if size == "small" else 8193
    m, tgt = cand_inputs(npos)
    return D.d_candidates(torch, ctx, D.dev_map(torch, m), tgt, npos, 3, npos)


@functools.lru_cache(maxsize=None)
def _geo():
    mean, cov = map_v1()
    return GS.geo_scene(mean, cov, gt_sync()["V1_01_easy"])


def _composite(torch, ctx, _):
    sc = _geo()
    s = _scene(torch, ctx, sc)
    r = covis.search_in_neighbors_from_map(ctx, api.Camera(), s["md"], s["bd"], s["cov"], dict(desc=s["kf_desc"]), sc["kf_row"], 5, stats=s["stats"],
                                           mp_replaced=s["rep"], mp_ref_kf=s["rk"], sizes=s["sizes"])
    h = _host(torch, s, r["sizes"])
    alive = h["mp_valid"] != 0
    for k in ("mp_desc", "mp_normal", "mp_max_dist", "mp_min_dist"):
        h[k] = h[k][alive]
    return dict(h, sizes=np.array(r["sizes"]), tgt=np.array(r["tgt_kf"]), counts=np.array(r["n_fused"] + r["n_attached"] + r["n_replaced"] + [r["n_cand"]]))


CALLS = {"graph": _graph, "graph_wide": _graph_wide, "fuse_candidates": _candidates, "search_in_neighbors_from_map": _composite}
OTHERS = ("mapping_pass_from_map", "cull_keyframes", "map_remove", "ba_window_build", "update_map_points")
_first = {}


def first_call(torch, name):
    if name not in _first:
        _first[name] = on_new_context(torch, lambda t, c: CALLS[name](t, c, "small"))
    return copy.deepcopy(_first[name])


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_other_map_entry_points(torch, name):
    fn = CALLS[name]
    ref = first_call(torch, name)
    ctx = new_context()
    try:
        same(run(lambda t, c: fn(t, c, "small"), torch, ctx), ref, (name, "first"))
        for other in CALLS.values():
            run(lambda t, c: other(t, c, "large"), torch, ctx)
        same(run(lambda t, c: fn(t, c, "small"), torch, ctx), ref, (name, "after the larger calls"))
        for other in OTHERS:
            run(BY_NAME[other].large, torch, ctx)
        run(lambda t, c: _add(t, c, "euroc"), torch, ctx)
        run(lambda t, c: _fuse(t, c, "euroc"), torch, ctx)
        same(run(lambda t, c: fn(t, c, "small"), torch, ctx), ref, (name, "after the other map entry points"))
    finally:
        close_context(ctx)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    fn = CALLS[name]
    ref = first_call(torch, name)
    ctx = new_context()
    try:
        for other in CALLS.values():
            run(lambda t, c: other(t, c, "large"), torch, ctx)
        ctx.set_option("test_scratch_fill", v)  # every block the context holds, now
        same(run(lambda t, c: fn(t, c, "small"), torch, ctx), ref, (name, "blocks filled with 0x%02X" % v))
    finally:
        close_context(ctx)
    same(on_new_context(torch, lambda t, c: fn(t, c, "small"), fill=v), ref, (name, "new context, blocks filled with 0x%02X as they are allocated" % v))


def test_timers_on(torch):
    refs = {name: first_call(torch, name) for name in CALLS}
    ctx = new_context()
    try:
        ctx.timing(True)
        for _ in range(2):
            for name, fn in CALLS.items():
                same(run(lambda t, c: fn(t, c, "small"), torch, ctx), refs[name], (name, "timers on"))
    finally:
        close_context(ctx)
