"""The C++ host mirror's depth-ordered walks (include/gmmloc_hip/gmm_adapter.hpp: createMapPointsFromStereo, createTemporalPoints,
processKeyFrameInMap) must give what the Python host gives through the same C-ABI: a g++-built driver (tests/cpp/key_frame_create_check.cpp)
takes the key-frame of tests/test_gpu_key_frame_create.py's scene - host vectors for the two walks, the resident map in capacity buffers for
the composite; every list it returns and every byte it leaves in the buffers is compared."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import cpp_driver
from tests import key_frame_create_cases as cc
from tests.gpu_helpers import T, stop_on_device_error  # noqa: F401 (the fixture is autouse here too)
from tests.test_gpu_key_frame_create import key_frame_scene
from tests.test_gpu_map_grow import refresh, upload, with_point_arrays

pytestmark = pytest.mark.gpu


def test_cpp_key_frame_create_matches_python_host(gpu, map_v1, gt_sync, tmp_path):
    torch, ctx = gpu
    exe = cpp_driver.build("key_frame_create_check", tmp_path)
    api.GMM(ctx, *map_v1).save(tmp_path / "m.gmm")
    g = api.GMM.load(ctx, tmp_path / "m.gmm")  # (the map both hosts read: the file)
    sc, m0, ba0, K, held, depth, cam = key_frame_scene(map_v1, gt_sync)
    th = np.float32(35.0 * cam.bf / cam.fx)
    NMP, (NKF, NFK), NOBS = len(m0["mp_valid"]), m0["kf_mp"].shape, len(m0["obs_kf"])
    NMPcap, OBScap = NMP + 300, NOBS + 300
    kf_desc = T(torch, sc["kf_desc"])
    md, bd, rk, sizes = upload(torch, with_point_arrays(m0, NMPcap), ba0, sc["mp_ref_kf"], NMPcap, OBScap)
    refresh(ctx, md, bd, rk, kf_desc, sizes)
    torch.cuda.synchronize()
    H = lambda t: t.cpu().numpy()
    outlier = (np.arange(NFK) % 5 == 2).astype(np.uint8)
    last = cc.last_rows(NFK)
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, NMPcap, OBScap, ba0["kf_first"], K, cam.width, cam.height], np.int32).tofile(fh)
        np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf], np.float64).tofile(fh)
        np.array([th], np.float32).tofile(fh)
        for a in (H(md["mp_valid"]), H(md["kf_valid"]), H(md["kf_mp"]), H(md["obs_ptr"]), H(md["obs_kf"]), H(bd["obs_feat"]), H(bd["kf_pose"]), H(bd["kf_twc"]),
                  H(bd["kf_uvr"]), H(bd["kf_oct"]), H(md["mp_pos"]), H(md["mp_normal"]), H(md["mp_max_dist"]), H(md["mp_min_dist"]), H(md["mp_desc"]),
                  H(bd["mp_assoc"]), H(rk), sc["kf_desc"], depth, held, outlier, last["last_pt"], last["last_observed"], last["last_valid"], last["last_desc"]):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    # the same sequence from Python
    uvr = bd["kf_uvr"][K]
    pose, uv = bd["kf_pose"][K][None].contiguous(), uvr[None, :, :2].contiguous()
    cand, ncand, _, _ = g.search2d(cam, pose, uv, k=5)
    row = torch.tensor([K], dtype=torch.int32, device="cuda")
    feats = dict(pose=pose, feat_uv=uv, feat_depth=T(torch, depth)[None], feat_oct=bd["kf_oct"][K][None].contiguous(), held=T(torch, held)[None])
    s = api.create_stereo_points(ctx, g, cam, api.Params(), dict(feats, feat_ur=uvr[None, :, 2].float().contiguous(), cand=cand, ncand=ncand, kf_row=row), NMP, 1,
                                 float(th))
    last_dev = {k: T(torch, v[None]) for k, v in last.items()}
    t = api.create_temporal_points(ctx, cam, dict(feats, last_outlier=T(torch, outlier)[None], feat_desc=kf_desc[K][None].contiguous()), last_dev, float(th))
    p = map_grow.process_key_frame_from_map(ctx, g, cam, api.Params(), md, bd, dict(desc=kf_desc), K, T(torch, depth), T(torch, held), float(th), sizes=sizes,
                                            mp_ref_kf=rk)
    torch.cuda.synchronize()
    n = int(s["n_new"][0])
    assert p["status"] == 0 and n > 20 and p["n_new"] == n and int(t["n_temp"][0]) > 20
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    eq = lambda dt, a: rd(dt, a.size).tobytes() == np.ascontiguousarray(a).tobytes()
    assert rd(np.int32, 1)[0] == n and eq(np.int32, H(s["stats"][0]))
    assert eq(np.int32, H(s["new_feat"][0, :n])) and eq(np.int32, H(s["new_assoc"][0, :n])) and eq(np.float64, H(s["new_pos"][0, :n]))
    assert eq(np.int32, H(s["feat_new"][0])) and eq(np.int32, H(cand[0])) and eq(np.int32, H(ncand[0]))
    assert eq(np.uint8, H(t["temp_flag"][0]))
    for k in ("last_pt", "last_observed", "last_valid", "last_desc"):
        assert eq(np.float64 if k == "last_pt" else np.uint8, H(last_dev[k][0])), k
    assert rd(np.int32, 6).tolist() == [p["sizes"][0], p["sizes"][2], p["n_attached"], p["n_skipped"], p["status"], n]
    assert eq(np.int32, H(p["stats"])) and eq(np.int32, H(p["feat_new"])) and eq(np.int32, H(p["cand"])) and eq(np.int32, H(p["ncand"]))
    for tns, dt in ((md["mp_valid"], np.uint8), (md["kf_valid"], np.uint8), (md["kf_mp"], np.int32), (md["obs_ptr"], np.int32), (md["obs_kf"], np.int32),
                    (bd["obs_feat"], np.int32), (md["mp_pos"], np.float64), (md["mp_normal"], np.float64), (md["mp_max_dist"], np.float32),
                    (md["mp_min_dist"], np.float32), (md["mp_desc"], np.uint8), (bd["mp_assoc"], np.int32), (rk, np.int32)):
        assert rd(dt, tns.numel()).tobytes() == H(tns).tobytes()
    assert out.read() == b""
