"""GPU: every case of tests/gmm_cases.py through gl_gmm_create (k_build_components, k_nbs), gl_knn3d (both kernels) and
GL_ASSOC_KNN5_EUCLID, against the declared outputs and the 60-digit values of tests/golden/gmm_cases_exact.npz.

Flags, graphs and k-NN indices equal the declared values.  The decomposition is held to the 60-digit values within
gmm_cases.DEVICE_BOUND (4x the CPU oracle's measured worst error, floor 8 units); cov_inv, det and flags stay bit-equal
to the oracle, and so does every other built array on these cases, which is asserted too.  The tests read the case
module and the npz only (no mpmath)."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import gmm_cases as gc

pytestmark = pytest.mark.gpu

FIELDS = dict(cov_inv=api.F_COV_INV, det=api.F_DET, scale=api.F_SCALE, axis=api.F_AXIS, sqrt_info=api.F_SQRT_INFO,
              flags=api.F_FLAGS, hgw=api.F_HGW, plane4=api.F_PLANE4)


@pytest.fixture(scope="module")
def exact():
    return gc.load_exact()


def device_build(g):
    return {k: g.get(f) for k, f in FIELDS.items()}


def oracle_build(oracle, mean, cov):
    h = oracle.gmm_create(mean, cov)
    out = oracle.gmm_get(h)
    oracle.gmm_destroy(h)
    out["hgw"] = gc.hgw_of(out["sqrt_info"])
    out["plane4"] = gc.plane4_of(out["axis"], np.asarray(mean, dtype=np.float64).reshape(-1, 3))
    return out


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_build_cases(gpu, oracle, exact, capsys):
    """every BUILD case in one map: declared flags, axes and planes; hgw and plane4 read back; the 60-digit values"""
    torch, ctx = gpu
    mean, cov = gc.build_map(gc.ALL_BUILD)
    got = device_build(api.GMM(ctx, mean, cov))
    worst = gc.check_build(got, exact[0], gc.ALL_BUILD, "device")
    ref = oracle_build(oracle, mean, cov)
    equal = {k: same(got[k], ref[k]) for k in FIELDS}
    with capsys.disabled():
        print("\ndevice, worst error per quantity: " + ", ".join("%s %.3g (%s)" % (q, v, n) for q, (v, n) in sorted(worst.items())))
        print("device bit-equal to the oracle: " + ", ".join("%s %s" % kv for kv in sorted(equal.items())))
    for q, (v, n) in worst.items():
        assert v <= gc.DEVICE_BOUND[q], (q, v, n)
    assert equal["cov_inv"] and equal["det"] and equal["flags"]
    # measured on the MI355X: every array of every case equals the oracle's bit for bit (the same expression order, and
    # sqrt and division correctly rounded on both sides), so that is held as well
    assert all(equal.values()), equal
    # hgw and plane4 are what the kernel stores for the BA edges: the same expressions on its own sqrt_info and axis
    assert same(got["hgw"], gc.hgw_of(got["sqrt_info"])) and same(got["plane4"], gc.plane4_of(got["axis"], mean))


@pytest.mark.parametrize("K", gc.BUILD_K_EDGES)
def test_build_block_edges(gpu, oracle, K):
    """the decisive case in the last slot of a map of 1, 127, 128, 129 components (k_build_components runs blocks of 128)"""
    torch, ctx = gpu
    mean, cov, flags = gc.build_edge_map(K)
    got = device_build(api.GMM(ctx, mean, cov))
    assert np.array_equal(got["flags"], flags)
    ref = oracle_build(oracle, mean, cov)
    assert same(got["cov_inv"], ref["cov_inv"]) and same(got["det"], ref["det"])
    c = gc.BUILD_BY_NAME["diag.in"]
    assert np.array_equal(got["plane4"][K - 1], [0.0, 1.0, 0.0, c["mean"][1]])  # the smallest entry is the second
    assert np.array_equal(got["plane4"][:K - 1], np.array([[1.0, 0.0, 0.0, float(i)] for i in range(K - 1)]).reshape(-1, 4))
    assert np.array_equal(got["hgw"][:K - 1], np.tile([1.0, 0, 0, 1, 0, 1], (K - 1, 1)))


def test_failed_cholesky_leaves_the_neighbours_rows_alone(gpu):
    torch, ctx = gpu
    good = ["cond1e6", "disc"]
    alone = device_build(api.GMM(ctx, *gc.build_map(good)))
    for bad in ("bad.indef", "bad.singular", "bad.inf", "bad.nan", "asym.lower"):
        mixed = device_build(api.GMM(ctx, *gc.build_map([good[0], bad, good[1]])))
        for k in FIELDS:
            assert np.array_equal(mixed[k][[0, 2]], alone[k]), (bad, k)
        assert np.isnan(mixed["sqrt_info"][1]).all() and np.isnan(mixed["hgw"][1]).all()
        assert mixed["flags"][1] == gc.BUILD_BY_NAME[bad]["flags"]


def test_build_through_save_and_load(gpu, exact, tmp_path):
    """saveGMMModel -> loadGMMModel transposes the covariance: the loaded map reads the other triangle, so asym.lower
    comes back as asym.saved with the other flag, and everything symmetric comes back with equal bits"""
    torch, ctx = gpu
    names = [n for n in gc.ALL_BUILD if not n.startswith("bad.")]
    mean, cov = gc.build_map(names)
    g = api.GMM(ctx, mean, cov)
    g.save(tmp_path / "cases.gmm")
    g2 = api.GMM.load(ctx, tmp_path / "cases.gmm")
    a, b = device_build(g), device_build(g2)
    assert np.array_equal(g2.get(api.F_COV).reshape(-1, 3, 3), cov.reshape(-1, 3, 3).transpose(0, 2, 1))
    swap = {"asym.lower": "asym.saved", "asym.saved": "asym.lower", "asym2.lower": "asym2.saved", "asym2.saved": "asym2.lower"}
    loaded = [swap.get(n, n) for n in names]
    assert [int(f) for f in b["flags"]] == [gc.BUILD_BY_NAME[n]["flags"] for n in loaded]
    worst = gc.check_build(b, exact[0], loaded, "loaded")
    for q, (v, n) in worst.items():
        assert v <= gc.DEVICE_BOUND[q], (q, v, n)
    sym = [i for i, n in enumerate(names) if n not in swap]
    for k in FIELDS:
        assert np.array_equal(a[k][sym], b[k][sym]), k


@pytest.mark.parametrize("name", [c["name"] for c in gc.GRAPH])
def test_graph_cases(gpu, oracle, exact, name):
    torch, ctx = gpu
    c = gc.GRAPH_BY_NAME[name]
    g = api.GMM(ctx, c["mean"], c["cov"], api.Params(neighbor_dist_thresh=c["thresh"]))
    ptr, col, dist = g.get(api.F_NBS_PTR), g.get(api.F_NBS_IDX), g.get(api.F_NBS_DIST)
    err = gc.check_graph(c, ptr, col, dist, exact[1][name], gc.graph_cond(c))
    assert err <= gc.DEVICE_BOUND["nbs_dist"], (name, err)
    assert g.lib.gl_gmm_nbs_count(g.h) == sum(len(r) for r in c["rows"])
    h = oracle.gmm_create(c["mean"], c["cov"])
    optr, ocol, odist = oracle.neighbours(h, c["thresh"])
    oracle.gmm_destroy(h)
    assert np.array_equal(ptr, optr) and np.array_equal(col, ocol)
    np.testing.assert_allclose(dist, odist, rtol=0, atol=1e-12)  # as test_neighbour_graph_matches_oracle holds the shipped maps


def _knn_both_kernels(torch):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return gc.KNN_WAVE_N + (16 * ncu + 1,)  # <= 16 x CUs queries: a wave per query; one more: a thread per query, partial last block


@pytest.mark.parametrize("name", [c["name"] for c in gc.KNN])
def test_knn_cases(gpu, name):
    """the declared indices and the exact distances from both kernels, for every k the case declares, the decisive query
    first, last and on either side of a block edge; the padding is (-1, +inf)"""
    torch, ctx = gpu
    c = gc.KNN_BY_NAME[name]
    K = len(c["mean"])
    g = api.GMM(ctx, c["mean"], np.tile(gc.I3, (K, 1)))
    for N in _knn_both_kernels(torch):
        for k in c["want"]:
            q, idx, dist = gc.knn_expected(c, N, k)
            gi, gd = g.knn3d(torch.from_numpy(q).cuda(), k)
            gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
            assert np.array_equal(gi, idx), (name, N, k, gi[0], idx[0])
            assert np.array_equal(gd, dist), (name, N, k)
            assert np.isposinf(gd[gi < 0]).all()
        # queryPoint / GL_ASSOC_KNN5_EUCLID: the first of the 5-NN and its chi2 (identity covariances: the squared distance)
        q, idx, dist = gc.knn_expected(c, N, 5)
        qi, qd = g.associate3d(torch.from_numpy(q).cuda(), api.ASSOC_KNN5_EUCLID)
        assert np.array_equal(qi.cpu().numpy(), idx[:, 0]), (name, N)
        assert np.array_equal(qd.cpu().numpy(), dist[:, 0]), (name, N)
        assert np.array_equal(g.queryPoint(torch.from_numpy(q).cuda()).cpu().numpy(), idx[:, 0])


def test_knn_through_a_loaded_map(gpu, tmp_path):
    """the same answers from a map that went through GMM.save / GMM.load"""
    torch, ctx = gpu
    c = gc.KNN_BY_NAME["tile.513"]
    K = len(c["mean"])
    api.GMM(ctx, c["mean"], np.tile(gc.I3, (K, 1))).save(tmp_path / "knn.gmm")
    g = api.GMM.load(ctx, tmp_path / "knn.gmm")
    for N in _knn_both_kernels(torch):
        for k in (1, 4, 8):
            q, idx, dist = gc.knn_expected(c, N, k)
            gi, gd = g.knn3d(torch.from_numpy(q).cuda(), k)
            assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(gd.cpu().numpy(), dist)
