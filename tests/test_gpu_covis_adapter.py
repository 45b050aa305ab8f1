"""The C++ host mirror's graph calls (include/gmmloc_hip/gmm_adapter.hpp: setResidentCovisibility, updateConnectionsInMap,
removeFromGraph, bestCovisible, searchInNeighborsInMap) must give what the Python host gives through the same C-ABI: a g++-built driver
(tests/cpp/covis_check.cpp) keeps a random map of tests/covis_cases.py and an empty graph on the device, updates every key-frame's
connections, removes three rows, updates some again, asks for two lists of best covisibles and for the targets and candidates of
searchInNeighbors; every list it returns and the graph it leaves on the device are compared bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api, covis
from tests import covis_cases as CC
from tests import covis_dev as D
from tests import cpp_driver

pytestmark = pytest.mark.gpu


def test_cpp_graph_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    exe = cpp_driver.build("covis_check", tmp_path)
    api.GMM(ctx, mean, cov).save(tmp_path / "m.gmm")
    m = CC.random_map(31)
    m["mp_valid"][np.random.default_rng(31).integers(0, CC.R_NMP, 40)] = 0
    NMP, (NKF, NFK), NOBS = len(m["mp_valid"]), m["kf_mp"].shape, len(m["obs_kf"])
    W, Ccap, kf_first, kf_idx, N = NKF, 3, 2, 9, 2
    upd, rm, upd2 = list(range(NKF)), [7, 2, 20, 8], [6, 9, 19, 21, 6]
    m["kf_valid"][rm[0]] = 0
    with open(tmp_path / "scene.bin", "wb") as fh:
        hd = [NMP, NKF, NFK, NOBS, W, Ccap, len(upd), len(rm), len(upd2), kf_first, 0, kf_idx, N, 0, 0, 0]
        # the key-frame of the lists: the one with the longest ordered list once the sequence has run (from the Python host, below)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        md = D.dev_map(torch, m)
        g = covis.covis_alloc(NKF, W)
        g["cov_kf"].fill_(-77)
        g["cov_w"].fill_(-77)
        want = []
        for k in upd:
            want.append(covis.covis_update(ctx, md, g, k, Ccap))
        res_rm = covis.covis_remove(ctx, g, NKF, T(np.array(rm, np.int32)), kf_first=kf_first)
        torch.cuda.synchronize()
        best_rm = g["best_cov"].cpu().numpy()[rm]
        for k in upd2:
            want.append(covis.covis_update(ctx, md, g, k, Ccap))
        kf_row = int(torch.argmax(g["cov_nord"]).item())
        hd[10] = kf_row
        np.array(hd, np.int32).tofile(fh)
        for a in (m["mp_valid"], m["kf_valid"], m["kf_mp"], m["obs_ptr"], m["obs_kf"], np.array(upd, np.int32), np.array(rm, np.int32), np.array(upd2, np.int32)):
            np.ascontiguousarray(a).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    H = lambda t: t.cpu().numpy()
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda cnt: np.fromfile(out, np.int32, cnt)

    def check_updates(ws):
        for i, w in enumerate(ws):
            res, n = H(w["result"]), int(H(w["n_conn"])[0])
            assert rd(4).tolist() == [n, res[0], res[1], res[2]], i
            k = min(n, Ccap)
            assert np.array_equal(rd(k), H(w["conn_kf"])[:k]) and np.array_equal(rd(k), H(w["conn_w"])[:k]), i

    check_updates(want[:len(upd)])
    res = H(res_rm)
    assert rd(4).tolist() == res.tolist() and res[0] == 3 and res[2] > 0  # (the key-frame with idx_ 0 is skipped)
    assert np.array_equal(rd(len(rm)), best_rm)
    check_updates(want[len(upd):])
    for n in (N, 0):
        b = covis.covis_best(ctx, g, NKF, T(np.array([kf_row], np.int32)), n, Ccap)
        k = min(int(H(b["n_conn"])[0]), Ccap)
        assert rd(1).tolist() == [k] and np.array_equal(rd(k), H(b["conn_kf"])[0, :k])
    t = covis.fuse_targets(ctx, g, md["kf_valid"], NKF, kf_row)
    n_tgt = int(H(t["n_tgt"])[0])
    c = covis.fuse_candidates(ctx, md, t["tgt_kf"], t["n_tgt"], kf_idx)
    n_cand = int(H(c["n_cand"])[0])
    assert n_tgt >= 3 and n_cand > 20
    assert rd(2).tolist() == [int(H(t["result"])[1]), n_tgt] and np.array_equal(rd(n_tgt), H(t["tgt_kf"])[:n_tgt])
    assert rd(3).tolist() == [int(H(t["result"])[1]) | int(H(c["result"])[1]), n_tgt, n_cand]
    assert np.array_equal(rd(n_tgt), H(t["tgt_kf"])[:n_tgt]) and np.array_equal(rd(n_cand), H(c["cand_mp"])[:n_cand])
    for k in ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov"):
        assert rd(H(g[k]).size).tobytes() == H(g[k]).tobytes(), k
    assert out.read() == b""
