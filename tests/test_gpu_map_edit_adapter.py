"""The C++ host mirror's edits of the resident map (include/gmmloc_hip/gmm_adapter.hpp: removeFromMap, cullKeyFrames) must give what
the Python host gives through the same C-ABI: a g++-built driver (tests/cpp/map_edit_check.cpp) keeps the `small` scene of
tests/map_edit_scenes.py (octaves clamped) on the device, erases observations and points, culls the covisible key-frames of one
key-frame and removes them; every list it returns and every row it leaves on the device is compared bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import cpp_driver
from tests import map_edit_scenes as ES
from tests.gpu_helpers import to_dev

pytestmark = pytest.mark.gpu


def test_cpp_map_edit_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    exe = cpp_driver.build("map_edit_check", tmp_path)
    api.GMM(ctx, mean, cov).save(tmp_path / "m.gmm")
    sc = ES.scene("small", True)
    m, ba = sc["m"], sc["ba"]
    NMP, NKF, NFK, NOBS = R._sizes(m)
    rm_mp, erase, _ = ES.removals(sc, 3)
    n_conn = [len(R.connections_vec(m, int(k))["conn_kf"]) for k in sc["rows"]]
    kf_row = int(sc["rows"][int(np.argmax(n_conn))])
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, kf_row, ba["kf_first"], len(erase), len(rm_mp)], np.int32).tofile(fh)
        np.array([sc["th_depth"]], np.float32).tofile(fh)
        for a in (m["mp_valid"], m["kf_valid"], m["kf_mp"], m["obs_ptr"], m["obs_kf"], ba["obs_feat"], ba["kf_uvr"], ba["kf_oct"], sc["kf_depth"], sc["mp_ref_kf"],
                  erase, rm_mp):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    # the same sequence from Python on the same rows
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    md, bd, rk = to_dev(torch, m), to_dev(torch, ba), T(sc["mp_ref_kf"].copy())
    e = api.map_remove(ctx, md, bd, erase_obs=T(erase), rm_mp=T(rm_mp), mp_ref_kf=rk)
    conn = api.update_connections(ctx, e["map"], torch.tensor([kf_row], dtype=torch.int32, device="cuda"), Ccap=64)
    c = api.cull_keyframes(ctx, e["map"], e["ba"], T(sc["kf_depth"]), sc["th_depth"], conn["conn_kf"], conn["n_conn"])
    k = api.map_remove(ctx, e["map"], e["ba"], rm_kf=c["cull_rows"][0], n_rm_kf=c["n_cull"], mp_ref_kf=rk)
    torch.cuda.synchronize()
    n = min(int(conn["n_conn"][0]), 64)
    nc = int(c["n_cull"][0])
    assert n >= 5 and nc >= 1 and e["n_dead"] > len(rm_mp) and k["nobs"] < e["nobs"] < NOBS
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    H = lambda t: t.cpu().numpy()
    for res in (e,):
        assert rd(np.int32, 3).tolist() == [res["nobs"], res["status"], res["n_dead"]] and np.array_equal(rd(np.int32, res["n_dead"]), H(res["dead_mp"]))
    assert rd(np.int32, 2).tolist() == [n, nc]
    assert np.array_equal(rd(np.int32, n), H(conn["conn_kf"])[0, :n]) and np.array_equal(rd(np.uint8, n), H(c["cull"])[0, :n])
    for key in ("num_mps", "num_redundant", "cand_status"):
        assert np.array_equal(rd(np.int32, n), H(c[key])[0, :n]), key
    assert np.array_equal(rd(np.int32, nc), H(c["cull_rows"])[0, :nc])
    assert rd(np.int32, 3).tolist() == [k["nobs"], k["status"], k["n_dead"]] and np.array_equal(rd(np.int32, k["n_dead"]), H(k["dead_mp"]))
    for t, cnt, dt in ((md["mp_valid"], NMP, np.uint8), (md["kf_valid"], NKF, np.uint8), (md["kf_mp"], NKF * NFK, np.int32), (md["obs_ptr"], NMP + 1, np.int32),
                       (k["map"]["obs_kf"], k["nobs"], np.int32), (k["ba"]["obs_feat"], k["nobs"], np.int32), (rk, NMP, np.int32)):
        assert rd(dt, cnt).tobytes() == H(t).tobytes()
    assert out.read() == b""
