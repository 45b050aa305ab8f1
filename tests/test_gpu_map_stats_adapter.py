"""The C++ host mirror's counter calls and removeMapPointsInMap (include/gmmloc_hip/gmm_adapter.hpp: setResidentMapStats, trackStats,
mergeStats, growStats, removeMapPointsInMap) must give what the Python host gives through the same C-ABI: a g++-built driver
(tests/cpp/map_stats_check.cpp) keeps the `small` scene of tests/map_edit_scenes.py and its counters on the device, counts two tracked
frames, merges a list of replacements, gives new rows their counters (across the capacity), appends to the candidate list and runs
removeMapPoints; every list it returns and every row it leaves on the device is compared bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api, map_stats
from tests import ba_window_ref as R
from tests import cpp_driver
from tests import map_edit_scenes as ES
from tests import map_stats_cases as SC
from tests.gpu_helpers import to_dev

pytestmark = pytest.mark.gpu


def test_cpp_map_stats_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    exe = cpp_driver.build("map_stats_check", tmp_path)
    api.GMM(ctx, mean, cov).save(tmp_path / "m.gmm")
    sc = ES.scene("small")
    m, ba = sc["m"], sc["ba"]
    NMP, NKF, NFK, NOBS = R._sizes(m)
    rng = np.random.default_rng(19)
    c = SC.random_case(sc, rng, 300)
    kf_idx = c["kf_idx"] if c["kf_idx"] is not None else np.arange(NKF, dtype=np.int32)
    NMPcap, n_new, n_already, n_merge, B, NF, NPcap = NMP + 8, 12, 20, 60, 2, 300, 500
    cand_cap = len(c["cand"]) + n_already + n_new + 5
    pad = lambda a, n, fill: np.concatenate([a, np.full(n - len(a), fill, np.int32)]).astype(np.int32)
    visible, found, ref_idx = pad(c["visible"], NMPcap, 0), pad(c["found"], NMPcap, 0), pad(c["ref_idx"], NMPcap, -1)
    cand = pad(c["cand"], cand_cap, -9)
    tr = dict(feat_mp=rng.integers(-1, NMP, (B, NF)).astype(np.int32), match_local=rng.integers(-1, NPcap, (B, NF)).astype(np.int32),
              outlier=(rng.random((B, NF)) < 0.2).astype(np.uint8), inview=(rng.random((B, NPcap)) < 0.5).astype(np.uint8),
              local_mp=rng.integers(0, NMP, (B, NPcap)).astype(np.int32), n_local_mp=np.array([NPcap, NPcap - 7], np.int32),
              counts2=np.zeros((B, 4), np.int32))
    src, tgt = rng.integers(0, NMP, n_merge).astype(np.int32), rng.integers(0, NMP, n_merge).astype(np.int32)
    new_ref_kf, already = rng.integers(-1, NKF + 1, n_new).astype(np.int32), rng.integers(0, NMP, n_already).astype(np.int32)
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, c["kf_row"], ba["kf_first"], NMPcap, cand_cap, len(c["cand"]), B, NF, NPcap, n_merge, n_new, n_already, 1],
                 np.int32).tofile(fh)
        for a in (m["mp_valid"], m["kf_valid"], m["kf_mp"], m["obs_ptr"], m["obs_kf"], ba["obs_feat"], ba["kf_uvr"], ba["kf_oct"], sc["mp_ref_kf"], visible,
                  found, ref_idx, kf_idx, cand, tr["feat_mp"], tr["match_local"], tr["outlier"], tr["inview"], tr["local_mp"], tr["n_local_mp"],
                  tr["counts2"], src, tgt, new_ref_kf, already):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    # the same sequence from Python on the same rows
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    md, bd, rk = to_dev(torch, {k: m[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}), to_dev(torch, ba), T(sc["mp_ref_kf"].copy())
    st = dict(visible=T(visible), found=T(found), ref_idx=T(ref_idx), kf_idx=T(kf_idx), cand=T(cand), n_cand=T(np.array([len(c["cand"])], np.int32)))
    d = to_dev(torch, tr)
    map_stats.map_stats_track(ctx, st, NMP, d["feat_mp"], d["match_local"], d["outlier"], d["inview"], d["local_mp"], d["n_local_mp"], d["counts2"])
    map_stats.map_stats_merge(ctx, st, NMP, T(src), T(tgt))
    s0 = map_stats.map_stats_new_points(ctx, st, NKF, NMP, T(new_ref_kf))
    a1 = map_stats.map_cand_append(ctx, st, rows=T(already))
    a2 = map_stats.map_cand_append(ctx, st, first=NMP, n=n_new)
    rr = map_stats.remove_map_points_from_map(ctx, md, bd, st, c["kf_row"], mp_ref_kf=rk)
    torch.cuda.synchronize()
    H = lambda t: t.cpu().numpy()
    grow = [int(H(s0)[0]) | int(H(a1)[1]) | int(H(a2)[1]), int(H(a2)[0])]
    res = H(rr["cull"]["result"]).tolist()
    n_old = sum(res[:3])
    assert grow == [map_stats.STATS_MP_TRUNCATED, len(c["cand"]) + n_already + n_new] and n_old == grow[1] and res[1] > 5 and res[0] > 5
    rem = rr["remove"]
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    assert rd(np.int32, 2).tolist() == grow
    assert rd(np.int32, 4).tolist() == res
    assert np.array_equal(rd(np.int32, n_old), H(rr["cull"]["verdict"])[:n_old]) and np.array_equal(rd(np.int32, res[1]), H(rr["cull"]["rm_mp"])[:res[1]])
    assert rd(np.int32, 3).tolist() == [rem["nobs"], rem["status"], rem["n_dead"]] and np.array_equal(rd(np.int32, rem["n_dead"]), H(rem["dead_mp"]))
    for name, t, cnt, dt in (("visible", st["visible"], NMPcap, np.int32), ("found", st["found"], NMPcap, np.int32), ("ref_idx", st["ref_idx"], NMPcap, np.int32),
                             ("n_cand", st["n_cand"], 1, np.int32), ("cand", st["cand"], cand_cap, np.int32), ("mp_valid", md["mp_valid"], NMP, np.uint8),
                             ("kf_mp", md["kf_mp"], NKF * NFK, np.int32), ("obs_ptr", md["obs_ptr"], NMP + 1, np.int32),
                             ("obs_kf", rem["map"]["obs_kf"], rem["nobs"], np.int32), ("obs_feat", rem["ba"]["obs_feat"], rem["nobs"], np.int32),
                             ("mp_ref_kf", rk, NMP, np.int32)):
        assert rd(dt, cnt).tobytes() == H(t).tobytes(), name
    assert out.read() == b""
