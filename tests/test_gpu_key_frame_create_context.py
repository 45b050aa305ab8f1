"""create_stereo_points, create_temporal_points and process_key_frame_from_map give the bits of the FIRST call of a new context whatever
the context has been through - the pass of tests/test_gpu_map_grow_context.py with its helpers: after larger calls of themselves, after
mapping_pass_from_map (which leaves its own bytes in the scratch block the stereo call uses), with every scratch block filled with 0x00 /
0xFF, and with the timers on."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import key_frame_create_cases as cc
from tests import keyframe_cases as kc
from tests.context_cases import BY_NAME, close_context, gmm_of, gt_sync, map_v1, new_context
from tests.test_gpu_context_state import on_new_context, run, torch  # noqa: F401 (torch: the module's fixture)
from tests.test_gpu_key_frame_create import T, generated, key_frame_scene, padded, stacked
from tests.test_gpu_map_grow_context import same

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


CALLS = {"create_stereo_points": (_stereo, "small", "large"), "create_temporal_points": (_temporal, "small", "large"),
         "process_key_frame_from_map": (_composite, None, None)}
_first = {}


def first_call(torch, name):
    if name not in _first:
        fn, small, _ = CALLS[name]
        _first[name] = on_new_context(torch, lambda t, c: fn(t, c, small))
    return _first[name]


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    """small, large, small on one context; then mapping_pass_from_map (large), then small again: each small equals the first call of a
    new context"""
    fn, small, large = CALLS[name]
    ref = first_call(torch, name)
    ctx = new_context()
    try:
        same(run(lambda t, c: fn(t, c, small), torch, ctx), ref, (name, "first"))
        run(lambda t, c: (CALLS["create_stereo_points"][0] if large is None else fn)(t, c, "large"), torch, ctx)
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
        run(lambda t, c: _stereo(t, c, "large"), torch, ctx)
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
