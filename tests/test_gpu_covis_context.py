"""The five calls of gmmloc_amd.covis and search_in_neighbors_from_map give the bits of the FIRST call of a new context whatever the
context has been through - the pass of tests/context_pass.py for this module: on a cold
context, after larger calls of themselves, after the other entry points of the resident map (which leave their marks in the two
scratch blocks these calls use), with every scratch block filled with 0x00 / 0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api, covis
from tests import covis_cases as CC
from tests import covis_dev as D
from tests import map_grow_scenes as GS
from tests.context_cases import BY_NAME, gt_sync, map_v1
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)
from tests.test_gpu_covis import _host, _scene, cand_inputs
from tests.test_gpu_map_grow_context import PASS as GROW  # (its prelude: map_add and map_fuse on the EuRoC-sized scene)

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
LARGE = tuple(at(fn, "large") for fn in CALLS.values())
PASS = Pass("covis", CALLS, small=dict.fromkeys(CALLS, "small"), larger=lambda name: LARGE,
            others=tuple(BY_NAME[other].large for other in OTHERS) + GROW.prelude, prelude=LARGE,
            legs=("after the larger calls", "after the other map entry points"))


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_other_map_entry_points(torch, name):
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
