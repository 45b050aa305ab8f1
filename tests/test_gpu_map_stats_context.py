"""The five calls of gmmloc_amd.map_stats and remove_map_points_from_map give the bits of the FIRST call of a new context whatever the
context has been through - the pass of tests/context_pass.py for this module, with the helpers of tests/context_cases.py: after larger calls of themselves, after mapping_pass_from_map (which leaves gl_map_remove's marks in the
scratch block gl_cull_map_points uses), with every scratch block filled with 0x00 / 0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from tests import map_edit_scenes as ES
from tests import map_stats_cases as SC
from tests.context_cases import BY_NAME
from tests.context_pass import Pass, after_legs, at, poisoned, run, timers_on, torch  # noqa: F401 (torch: the module's fixture)
from tests.test_gpu_map_stats import composite, device_cull, device_merge, device_track, make_stats

pytestmark = pytest.mark.gpu

SIZES = {"tiny": 40, "small": 4097}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    sc = ES.scene(name)
    return sc, SC.random_case(sc, np.random.default_rng(61), SIZES[name])


def _cull(torch, ctx, name):
    sc, c = _inputs(name)
    v, kept, rm, res = device_cull(torch, ctx, sc["m"], sc["ba"], c, c["cand"], c["kf_row"], cand_cap=len(c["cand"]) + 3)
    return dict(verdict=np.array(v), kept=np.array(kept), rm_mp=np.array(rm), result=np.array(res))


def _composite(torch, ctx, name):
    sc, c = _inputs(name)
    r, rk, g = composite(torch, ctx, sc, c)
    nobs = r["remove"]["nobs"]
    h = lambda t: t.cpu().numpy()
    return dict(mp_valid=h(r["remove"]["map"]["mp_valid"]), kf_mp=h(r["remove"]["map"]["kf_mp"]), obs_ptr=h(r["remove"]["map"]["obs_ptr"]),
                obs_kf=h(r["remove"]["map"]["obs_kf"])[:nobs], obs_feat=h(r["remove"]["ba"]["obs_feat"])[:nobs], mp_ref_kf=h(rk),
                obs_new_pos=h(r["remove"]["obs_new_pos"]), dead_mp=h(r["remove"]["dead_mp"]), cand=g.host("cand"), n_cand=g.host("n_cand"),
                verdict=h(r["cull"]["verdict"]), rm_mp=h(r["cull"]["rm_mp"]), result=h(r["cull"]["result"]))


def _counters(torch, ctx, name):
    """track, merge, new points and append, which take no scratch: the hand-built cases (small) or long random lists (large)"""
    from gmmloc_amd import map_stats
    big = name != "tiny"
    rng = np.random.default_rng(17)
    t, a = SC.TRACK, SC.track_arrays()
    NMP = t["NMP"]
    if big:
        NMP, B, NF, NP = 5000, 4, 1200, 3000
        a = dict(feat_mp=rng.integers(-1, NMP, (B, NF)).astype(np.int32), match_local=rng.integers(-1, NP, (B, NF)).astype(np.int32),
                 outlier=(rng.random((B, NF)) < 0.2).astype(np.uint8), inview=(rng.random((B, NP)) < 0.5).astype(np.uint8),
                 local_mp=rng.integers(0, NMP, (B, NP)).astype(np.int32), n_local_mp=np.full(B, NP, np.int32), counts2=np.zeros((B, 4), np.int32))
    g, st = make_stats(torch, [1] * NMP, [1] * NMP, [-1] * NMP, cand=[3, 4], cand_cap=NMP)
    vis, fnd = device_track(torch, ctx, g, st, NMP, a)
    c = SC.MERGE
    src, tgt = (rng.integers(0, NMP, 3000), rng.integers(0, NMP, 3000)) if big else (c["src"], c["tgt"])
    mv, mf = device_merge(torch, ctx, vis[:NMP] if big else c["visible"], fnd[:NMP] if big else c["found"], NMP if big else c["NMP"], src, tgt)
    n_new = NMP // 2
    def call(torch, ctx):
        ref_kf = torch.from_numpy(rng.integers(-1, 9, n_new).astype(np.int32)).cuda()
        status = map_stats.map_stats_new_points(ctx, st, 8, NMP - n_new + 1, ref_kf)
        res = map_stats.map_cand_append(ctx, st, first=NMP - n_new, n=n_new)
        torch.cuda.synchronize()
        return status.cpu().numpy(), res.cpu().numpy()
    status, res = run(call, torch, ctx)
    g.check()
    return dict(visible=np.array(vis), found=np.array(fnd), merged_visible=np.array(mv), merged_found=np.array(mf), status=status, append=res,
                new_visible=g.host("visible"), new_ref_idx=g.host("ref_idx"), cand=g.host("cand"), n_cand=g.host("n_cand"))


CALLS = {"counters": _counters, "cull_map_points": _cull, "remove_map_points_from_map": _composite}
PASS = Pass("map_stats", CALLS, small=dict.fromkeys(CALLS, "tiny"), larger=lambda name: (at(CALLS[name], "small"),),
            others=(BY_NAME["mapping_pass_from_map"].large,), prelude=(at(_composite, "small"),))


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
