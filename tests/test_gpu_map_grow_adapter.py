"""The C++ host mirror's additions to the resident map (include/gmmloc_hip/gmm_adapter.hpp: setResidentMapCapacity, addToMap,
fuseObservationsInMap) must give what the Python host gives through the same C-ABI: a g++-built driver (tests/cpp/map_grow_check.cpp)
keeps the `small` scene of tests/map_grow_scenes.py on the device in capacity buffers, adds a key-frame's rows, points and observations
and applies a list of fuse matches; every list it returns and every byte it leaves in the buffers is compared."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import cpp_driver
from tests import map_edit_scenes as ES
from tests import map_grow_ref as G
from tests import map_grow_scenes as GS
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse here too)
from tests.test_gpu_map_grow import upload

pytestmark = pytest.mark.gpu


def test_cpp_map_grow_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    exe = cpp_driver.build("map_grow_check", tmp_path)
    api.GMM(ctx, mean, cov).save(tmp_path / "m.gmm")
    m, ba, ref_kf, ls = GS.add_lists(ES.scene("small", True), 2)
    NMP, (NKF, NFK), NOBS = len(m["mp_valid"]), m["kf_mp"].shape, len(m["obs_kf"])
    att, new = ls["attach"], ls["new_mp"]
    # the fuse list is made on the model's grown map: an input of both routes
    rows1, res1 = G.map_add(m, ba, ref_kf, new, ls["new_kf"], att, ls["walk_kf"])
    m1, ba1 = G.apply_rows(m, ba, rows1, dict(mp_pos=new["pos"]))
    kf, cand, best = GS.fuse_lists(dict(m=m1, ba=ba1), 1)
    NMPcap, OBScap = res1[0] + 9, res1[1] + len(cand) + 9
    md, bd, rk, sizes = upload(torch, m, ba, ref_kf, NMPcap, OBScap)
    H = lambda t: t.cpu().numpy()
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, NMPcap, OBScap, ba["kf_first"], len(new["pos"]), len(ls["new_kf"]), len(att), len(ls["walk_kf"]), kf, len(cand)],
                 np.int32).tofile(fh)
        for a in (H(md["mp_valid"]), H(md["kf_valid"]), H(md["kf_mp"]), H(md["obs_ptr"]), H(md["obs_kf"]), H(bd["obs_feat"]), ba["kf_uvr"], H(md["mp_pos"]),
                  H(bd["mp_assoc"]), H(rk), new["pos"], new["assoc"], new["ref_kf"], ls["new_kf"], att[:, 0], att[:, 1], att[:, 2], ls["walk_kf"], cand, best):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    # the same sequence from Python on the same buffers
    T = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()
    a = map_grow.map_add(ctx, md, bd, sizes, new_mp=dict(pos=T(new["pos"], np.float64), assoc=T(new["assoc"]), ref_kf=T(new["ref_kf"])), new_kf=T(ls["new_kf"]),
                         attach=dict(mp=T(att[:, 0]), kf=T(att[:, 1]), feat=T(att[:, 2])), walk_kf=T(ls["walk_kf"]), mp_ref_kf=rk)
    f = map_grow.map_fuse(ctx, md, bd, kf, T(cand), T(best), sizes=a["sizes"])
    torch.cuda.synchronize()
    assert a["status"] == 0 and f["status"] == 0 and a["n_attached"] > 20 and a["n_already"] >= 1 and f["n_replaced"] >= 3 and f["n_attached"] >= 1
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    assert rd(np.int32, 6).tolist() == [a["sizes"][0], a["sizes"][2], a["n_attached"], a["n_skipped"], a["n_already"], a["status"]]
    assert np.array_equal(rd(np.int32, a["n_already"]), H(a["already_mp"]))
    assert rd(np.int32, 5).tolist() == [f["sizes"][2], f["n_fused"], f["n_attached"], f["n_replaced"], f["status"]]
    assert np.array_equal(rd(np.int32, f["n_replaced"]), H(f["repl_src"])) and np.array_equal(rd(np.int32, f["n_replaced"]), H(f["repl_tgt"]))
    for t, dt in ((md["mp_valid"], np.uint8), (md["kf_valid"], np.uint8), (md["kf_mp"], np.int32), (md["obs_ptr"], np.int32), (md["obs_kf"], np.int32),
                  (bd["obs_feat"], np.int32), (md["mp_pos"], np.float64), (bd["mp_assoc"], np.int32), (rk, np.int32)):
        assert rd(dt, t.numel()).tobytes() == H(t).tobytes()
    assert out.read() == b""
