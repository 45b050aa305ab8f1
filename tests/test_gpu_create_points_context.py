"""create_map_points_on_map (gl_create_map_points_from_map alone) and create_map_points_from_map give the bits of the FIRST call of a new
context whatever the context has been through - the pass of tests/context_pass.py for these two: after larger
calls of themselves, after every other map entry point and the three per-pair pieces (which leave their own bytes in the scratch blocks
the loop's stages use), with every scratch block filled with 0x00 / 0xFF, and with the timers on."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import create_points_cases as cc
from tests.context_cases import BY_NAME
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)
from tests.gpu_helpers import T
from tests.test_gpu_create_points import BA_KEYS, MAP_KEYS, resident, snapshot

pytestmark = pytest.mark.gpu

SIZES = {"small": (65, 6, 41, 4), "large": (257, 12, 9, 10)}  # NFK, key-frames, seed, nn
OTHERS = ("update_map_points", "ba_window_build", "ba_window_apply", "joint_optimization_from_map", "cull_keyframes", "map_remove", "mapping_pass_from_map",
          "search_for_triangulation_gather", "create_map_points", "track_frame_chain_map")


def _loop(torch, ctx, size):
    NFK, n_kf, seed, nn = SIZES[size]
    sc = cc.generated(NFK, n_kf, seed)
    g = api.GMM(ctx, sc.mean, sc.cov.reshape(-1, 9))
    try:
        cam = api.Camera(**sc.cam)
        o = map_grow.create_map_points_on_map(ctx, g, cam, api.Params(), {k: T(torch, sc.map[k]) for k in MAP_KEYS}, {k: T(torch, sc.ba[k]) for k in BA_KEYS},
                                              {k: T(torch, v) for k, v in sc.kt.items()}, 0, T(torch, np.arange(1, n_kf, dtype=np.int32)),
                                              T(torch, np.array([n_kf - 1], np.int32)), n_nb=nn, mb=map_grow.default_mb(cam), mp_base=sc.NMP)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in o.items()}
        n = int(h["n_new"][0])
        assert n > 10
        # (the entries behind the counts are the caller's: not compared)
        return {k: (v[:n] if v.shape[0] == sc.NFK and k.startswith("new_") else v[:2 * n] if k.startswith("att_") else v) for k, v in h.items()}
    finally:
        ctx.synchronize()
        g.close()


def _composite(torch, ctx, _):
    from tests.test_gpu_map_grow import refresh
    sc = cc.generated(257, 6, 23)
    g = api.GMM(ctx, sc.mean, sc.cov.reshape(-1, 9))
    try:
        ktd = {k: T(torch, v) for k, v in sc.kt.items()}
        md, bd, rk, sizes = resident(torch, sc, 600, 1200)
        refresh(ctx, md, bd, rk, ktd["desc"], sizes)
        r = map_grow.create_map_points_from_map(ctx, g, api.Camera(**sc.cam), api.Params(), md, bd, ktd, 0, nn=4, sizes=sizes, mp_ref_kf=rk)
        assert r["status"] == 0 and r["n_new"] > 10
        out = snapshot(torch, md, bd, rk)
        out.update(sizes=np.array(r["sizes"]), new_type=r["new_type"].cpu().numpy(), new_nb=r["new_nb"].cpu().numpy(), feat_new=r["feat_new"].cpu().numpy(),
                   nb_stats=r["nb_stats"].cpu().numpy())
        return out
    finally:
        ctx.synchronize()
        g.close()


CALLS = {"create_map_points_on_map": _loop, "create_map_points_from_map": _composite}
PASS = Pass("create_points", CALLS, small={"create_map_points_on_map": "small", "create_map_points_from_map": None},
            larger=lambda name: (at(_loop, "large"),), others=tuple(BY_NAME[other].large for other in OTHERS), prelude=(at(_loop, "large"),),
            legs=("after the larger call", "after the other entry points"))


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_other_entry_points(torch, name):
    """small, large, small on one context; then every other map entry point and the per-pair pieces (large), then small again: each small
    equals the first call of a new context"""
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
