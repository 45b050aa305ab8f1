"""The C++ host mirror's createMapPoints on the resident map (include/gmmloc_hip/gmm_adapter.hpp: setResidentKeyFrameTables,
createMapPointsInMap) must give what the Python host gives through the same C-ABI: a g++-built driver (tests/cpp/create_points_check.cpp)
takes the generated key-frames of tests/test_gpu_create_points.py in capacity buffers; every list it returns and every byte it leaves in
the buffers is compared with map_grow.create_map_points_from_map's."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import cpp_driver
from tests import create_points_cases as cc
from tests.gpu_helpers import T, stop_on_device_error  # noqa: F401 (the fixture is autouse here too)
from tests.test_gpu_create_points import resident
from tests.test_gpu_map_grow import refresh

pytestmark = pytest.mark.gpu


def test_cpp_create_points_matches_python_host(gpu, tmp_path):
    torch, ctx = gpu
    exe = cpp_driver.build("create_points_check", tmp_path)
    sc, nn = cc.generated(257, 6, 23), 4
    api.GMM(ctx, sc.mean, sc.cov.reshape(-1, 9)).save(tmp_path / "m.gmm")
    g = api.GMM.load(ctx, tmp_path / "m.gmm")  # (the map both hosts read: the file)
    cam = api.Camera(**sc.cam)
    mb = np.float32(map_grow.default_mb(cam))
    ktd = {k: T(torch, v) for k, v in sc.kt.items()}
    md, bd, rk, sizes = resident(torch, sc, 300, 600)
    refresh(ctx, md, bd, rk, ktd["desc"], sizes)
    torch.cuda.synchronize()
    NMP, NKF, NOBS = sizes
    NFK, NMPcap, OBScap = sc.NFK, md["obs_ptr"].shape[0] - 1, md["obs_kf"].shape[0]
    H = lambda t: t.cpu().numpy()
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, NMPcap, OBScap, -1, 0, cam.width, cam.height, nn, sc.kt["node_id"].shape[1], sc.kt["cand"].shape[2]], np.int32).tofile(fh)
        np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf], np.float64).tofile(fh)
        np.array([mb], np.float32).tofile(fh)
        for a in (H(md["mp_valid"]), H(md["kf_valid"]), H(md["kf_mp"]), H(md["obs_ptr"]), H(md["obs_kf"]), H(bd["obs_feat"]), H(bd["kf_pose"]), H(bd["kf_twc"]),
                  H(bd["kf_uvr"]), H(bd["kf_oct"]), H(md["mp_pos"]), H(md["mp_normal"]), H(md["mp_max_dist"]), H(md["mp_min_dist"]), H(md["mp_desc"]),
                  H(bd["mp_assoc"]), H(rk)) + tuple(sc.kt[k] for k in ("angle", "desc", "depth", "nnode", "node_id", "node_ptr", "node_idx", "cand", "ncand")):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    p = map_grow.create_map_points_from_map(ctx, g, cam, api.Params(), md, bd, ktd, 0, nn=nn, mb=float(mb), sizes=sizes, mp_ref_kf=rk)
    torch.cuda.synchronize()
    n = p["n_new"]
    assert p["status"] == 0 and n > 10
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    eq = lambda dt, a: rd(dt, a.size).tobytes() == np.ascontiguousarray(a).tobytes()
    assert rd(np.int32, 7).tolist() == [p["sizes"][0], p["sizes"][2], p["n_attached"], p["n_skipped"], p["status"], n, 0]
    assert eq(np.int32, H(p["new_type"])) and eq(np.int32, H(p["new_nb"])) and eq(np.int32, H(p["feat_new"])) and eq(np.int32, H(p["nb_stats"]))
    for tns, dt in ((md["mp_valid"], np.uint8), (md["kf_valid"], np.uint8), (md["kf_mp"], np.int32), (md["obs_ptr"], np.int32), (md["obs_kf"], np.int32),
                    (bd["obs_feat"], np.int32), (md["mp_pos"], np.float64), (md["mp_normal"], np.float64), (md["mp_max_dist"], np.float32),
                    (md["mp_min_dist"], np.float32), (md["mp_desc"], np.uint8), (bd["mp_assoc"], np.int32), (rk, np.int32)):
        assert rd(dt, tns.numel()).tobytes() == H(tns).tobytes()
    assert out.read() == b""
