"""The C++ host mirror's map-resident local BA (include/gmmloc_hip/gmm_adapter.hpp: flattenMap, flattenMapBa, setResidentMap,
jointOptimizationFromMap) must give what the Python host gives through the same C-ABI: a g++-built driver
(tests/cpp/ba_window_check.cpp) flattens the geometric scene of tests/ba_window_scenes.py, keeps it on the device, runs one key-frame's
local BA from it, and every row it returns or leaves on the device is compared bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import cpp_driver

pytestmark = pytest.mark.gpu


def test_cpp_from_map_matches_python_host(gpu, map_v1, gt_sync, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    exe = cpp_driver.build("ba_window_check", tmp_path)
    g0 = api.GMM(ctx, mean, cov)
    g0.save(tmp_path / "m.gmm")
    g = api.GMM.load(ctx, tmp_path / "m.gmm")
    m, ba, kf = S.geometric_scene(mean, cov, gt_sync["V1_01_easy"], cam)
    NMP, NKF, NFK, NOBS = R._sizes(m)
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, kf, ba["kf_first"], cam.width, cam.height, 0], np.int32).tofile(fh)
        np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf], np.float64).tofile(fh)
        for a in (m["mp_valid"], m["kf_valid"], m["kf_mp"], m["mp_pos"], ba["kf_pose"], ba["kf_uvr"], ba["kf_oct"], ba["mp_assoc"]):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, n: np.fromfile(out, dt, n)
    # the rows the adapter flattened: the same observations as the scene's CSR (there in no particular order, here key-frames ascending)
    obs_ptr, obs_kf, obs_feat = rd(np.int32, NMP + 1), rd(np.int32, NOBS), rd(np.int32, NOBS)
    assert np.array_equal(obs_ptr, m["obs_ptr"])
    pt = np.repeat(np.arange(NMP), np.diff(obs_ptr))
    order = lambda k, f: np.lexsort((f, k, pt))
    a, b = order(m["obs_kf"], ba["obs_feat"]), order(obs_kf, obs_feat)
    assert np.array_equal(m["obs_kf"][a], obs_kf[b]) and np.array_equal(ba["obs_feat"][a], obs_feat[b]) and (np.diff(obs_kf)[np.diff(pt) == 0] > 0).all()
    twc = rd(np.float64, NKF * 3).reshape(NKF, 3)
    assert twc.tobytes() == np.stack([R.twc_of(p) for p in ba["kf_pose"]]).tobytes()
    # the same call from Python on the same rows
    m2, ba2 = dict(m, obs_kf=obs_kf), dict(ba, obs_feat=obs_feat, kf_twc=twc)
    T = lambda d: {k: (torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x) for k, x in d.items()}
    md, bd = T(m2), T(ba2)
    ref = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, (24, 24, 2048, 16384))
    torch.cuda.synchronize()
    P, F, L, nobs, status, iters, ne = rd(np.int32, 7)
    assert (P, F, L, nobs, status) == (ref["P"], ref["F"], ref["L"], ref["nobs"], ref["status"]) and iters == int(ref["iters"][0]) > 0
    assert 4 <= P <= 20 and F >= 1 and L >= 300
    assert np.array_equal(rd(np.int32, P + F), ref["win_kf"].cpu().numpy()) and np.array_equal(rd(np.int32, L), ref["win_mp"].cpu().numpy())
    assert np.array_equal(rd(np.uint8, L), ref["assoc_dropped"].cpu().numpy())
    assert ne == len(ref["erase_obs"]) > 0 and np.array_equal(rd(np.int32, ne), ref["erase_obs"].cpu().numpy())
    for t, n, dt in ((bd["kf_pose"], NKF * 7, np.float64), (bd["kf_twc"], NKF * 3, np.float64), (md["mp_pos"], NMP * 3, np.float64), (bd["mp_assoc"], NMP, np.int32)):
        assert rd(dt, n).tobytes() == t.cpu().numpy().tobytes()
    assert out.read() == b""
    assert not np.array_equal(bd["kf_pose"].cpu().numpy(), ba["kf_pose"])
