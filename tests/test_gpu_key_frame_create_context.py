"""create_stereo_points, create_temporal_points and process_key_frame_from_map give the bits of the FIRST call of a new context whatever
the context has been through - the pass of tests/context_pass.py for these three: after larger calls of themselves, after
mapping_pass_from_map (which leaves its own bytes in the scratch block the stereo call uses), with every scratch block filled with 0x00 /
0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import key_frame_create_cases as cc
from tests import keyframe_cases as kc
from tests.context_cases import BY_NAME, gmm_of, gt_sync, map_v1
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)
from tests.gpu_helpers import T
from tests.test_gpu_key_frame_create import generated, key_frame_scene, padded, stacked

pytestmark = pytest.mark.gpu

SIZES = {"small": (102, 1), "large": (api.STEREO_WALK_MAX, 3)}


@functools.lru_cache(maxsize=None)
def _frames(size):
    NF, B = SIZES[size]
    return [padded(generated(NF - 7 * b), NF, 3 * b) for b in range(B)]


def _stereo(torch, ctx, size):
    g = api.GMM(ctx, *kc.mk_map(cc.MAP_MOVE))
    try:
        fr = _frames(size)
        r = api.create_stereo_points(ctx, g, api.Camera(**kc.CAM5), api.Params(), stacked(torch, fr, list(range(len(fr)))), 50, 1, float(cc.TH), want_pts0=True)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}
    finally:
        ctx.synchronize()
        g.close()


def _temporal(torch, ctx, size):
    fr = _frames(size)
    last = {k: T(torch, np.stack([cc.last_rows(len(f["held"]))[k] for f in fr])) for k in api.TEMPORAL_LAST_DTYPES}
    r = api.create_temporal_points(ctx, api.Camera(**kc.CAM5), {k: T(torch, np.stack([f[k] for f in fr])) for k in api.TEMPORAL_IN_DTYPES}, last, float(cc.TH))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(r, **last).items()}


@functools.lru_cache(maxsize=None)
def _scene():
    return key_frame_scene(map_v1(), gt_sync())


def _composite(torch, ctx, _):
    from tests.test_gpu_map_grow import refresh, upload, with_point_arrays
    sc, m0, ba0, K, held, depth, cam = _scene()
    NMP, NOBS = len(m0["mp_valid"]), len(m0["obs_kf"])
    kf_desc = T(torch, sc["kf_desc"])
    md, bd, rk, sizes = upload(torch, with_point_arrays(m0, NMP + 400), ba0, sc["mp_ref_kf"], NMP + 400, NOBS + 400)
    refresh(ctx, md, bd, rk, kf_desc, sizes)
    r = map_grow.process_key_frame_from_map(ctx, gmm_of(ctx), cam, api.Params(), md, bd, dict(desc=kf_desc), K, T(torch, depth), T(torch, held), 35.0 * cam.bf / cam.fx,
                                            sizes=sizes, mp_ref_kf=rk)
    torch.cuda.synchronize()
    assert r["status"] == 0 and r["n_new"] > 20
    out = {"map." + k: v.cpu().numpy() for k, v in md.items()}
    out.update({"ba." + k: v.cpu().numpy() for k, v in bd.items() if hasattr(v, "cpu")})
    out.update(mp_ref_kf=rk.cpu().numpy(), sizes=np.array(r["sizes"]), feat_new=r["feat_new"].cpu().numpy(), stats=r["stats"].cpu().numpy(),
               cand=r["cand"].cpu().numpy(), ncand=r["ncand"].cpu().numpy())
    return out


CALLS = {"create_stereo_points": _stereo, "create_temporal_points": _temporal, "process_key_frame_from_map": _composite}
# (the composite has one size: the larger call is the stereo walk's)
PASS = Pass("key_frame_create", CALLS, small={"create_stereo_points": "small", "create_temporal_points": "small", "process_key_frame_from_map": None},
            larger=lambda name: (at(_stereo if name == "process_key_frame_from_map" else CALLS[name], "large"),),
            others=(BY_NAME["mapping_pass_from_map"].large,), prelude=(at(_stereo, "large"),))


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
