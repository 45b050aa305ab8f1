"""The three rebuilds of the CSR on a map whose ranges OVERLAP: obs_ptr = {0, 4, 0, 4} with NOBS = 4, so points 0 and 2 both claim
[0, 4) and point 1 has a reversed range.  The scanned places then run past NOBS (0, 4, 4 -> a total of 8), and the move must still
store nothing at or behind its limit: NOBS for gl_map_remove, the OBScap PASSED for gl_map_add and gl_map_fuse.  obs_kf / obs_feat are
allocated with 64 entries and OBScap = 5 is passed, so a move without the limit shows in the sentinels and still stays inside the
allocation.  What a malformed CSR compacts to is not defined, and nothing here defines it: only what must NOT be written is held."""
import ctypes as C

import numpy as np
import pytest

from gmmloc_amd import _lib, api
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.gpu_helpers import stop_on_device_error  # noqa: F401  (autouse: the same after every test of this module)

pytestmark = pytest.mark.gpu

SENT = -9
NMP, NKF, NFK, NOBS, ALLOC, OBSCAP = 3, 2, 4, 4, 64, 5


def the_map():
    obs_kf, obs_feat = np.full(ALLOC, SENT, np.int32), np.full(ALLOC, SENT, np.int32)
    obs_kf[:NOBS], obs_feat[:NOBS] = (0, 1, 0, 1), (0, 1, 2, 3)
    kf_mp = np.full((NKF, NFK), -1, np.int32)
    kf_mp[obs_kf[:NOBS], obs_feat[:NOBS]] = 0
    kf_uvr = np.zeros((NKF, NFK, 3))
    kf_uvr[..., 2] = -1.0
    return dict(mp_valid=np.ones(NMP, np.uint8), kf_valid=np.ones(NKF, np.uint8), kf_mp=kf_mp, obs_ptr=np.array([0, 4, 0, 4], np.int32), obs_kf=obs_kf,
                obs_feat=obs_feat, kf_uvr=kf_uvr)


def on_device(gpu, call):
    """call(lib, ctx handle, sizes + edit struct, kf_uvr pointer, z) on a fresh upload -> (its return, the map before, the map after)"""
    torch, ctx = gpu
    before = the_map()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in before.items()}
    ed = _lib.gl_map_edit()
    for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat"):
        setattr(ed, k, api._ptr(dev[k]))
    z = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    def go(torch, ctx):
        ctx._enter()
        try:
            r = call(ctx.lib, ctx.h, C.byref(ed), api._ptr(dev["kf_uvr"]), z)
        finally:
            ctx._exit()
        torch.cuda.synchronize()
        return r
    got = run(go, torch, ctx)
    return got, before, {k: v.cpu().numpy() for k, v in dev.items()}


def test_fuse_writes_nothing_at_or_behind_the_capacity(gpu):
    def call(lib, h, ed, uvr, z):
        res, cand, best = z(5), z(1), z(1) - 1  # (best_idx = {-1}: no match, the rebuild runs all the same)
        fo = _lib.gl_map_fuse_out()
        fo.result = api._ptr(res)
        return lib.gl_map_fuse(h, NMP, NKF, NFK, NOBS, OBSCAP, ed, uvr, 0, 1, api._ptr(cand), api._ptr(best), C.byref(fo)), res
    (rc, _), before, after = on_device(gpu, call)
    assert rc == 0
    for k in ("obs_kf", "obs_feat"):
        assert (after[k][OBSCAP:] == SENT).all(), (k, after[k][:12])
        assert np.array_equal(after[k][:NOBS], before[k][:NOBS]), (k, after[k][:12])


def test_add_over_the_capacity_writes_nothing(gpu):
    def call(lib, h, ed, uvr, z):
        res = z(6)
        ls, o = _lib.gl_map_add_lists(), _lib.gl_map_add_out()
        o.result = api._ptr(res)
        return lib.gl_map_add(h, NMP, NKF, NFK, NOBS, NMP, OBSCAP, ed, None, None, C.byref(ls), C.byref(o)), res
    (rc, res), before, after = on_device(gpu, call)
    res = res.cpu().numpy()
    assert rc == 0 and res[5] & 1, res  # (GL_MAP_GROW_OBS_TRUNCATED)
    assert res[1] == 8, res
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), (k, after[k].ravel()[:12])


def test_remove_writes_nothing_at_or_behind_nobs(gpu):
    def call(lib, h, ed, uvr, z):
        res = z(3)
        ls, o = _lib.gl_map_remove_lists(), _lib.gl_map_remove_out()
        o.result = api._ptr(res)
        return lib.gl_map_remove(h, NMP, NKF, NFK, NOBS, ed, uvr, -1, C.byref(ls), C.byref(o)), res
    (rc, _), before, after = on_device(gpu, call)
    assert rc == 0
    for k in ("obs_kf", "obs_feat"):
        assert (after[k][NOBS:] == SENT).all(), (k, after[k][:12])
