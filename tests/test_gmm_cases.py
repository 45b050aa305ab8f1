"""CPU: tests/gmm_cases.py against the C++ oracle, oracle/numpy_ref.py, the 60-digit values of
tests/golden/gmm_cases_exact.npz and, where oracle/_ref has it, the reference's own nanoflann.

The oracle runs the same cyclic Jacobi, cofactor inverse and Cholesky as the kernels, so equality with it says nothing about
whether a decomposition is right: here both are held to the declared outputs and to the 60-digit values.  Every threshold
case is shown to lie on its declared side in 60-digit arithmetic with a margin of at least 20x the oracle's own error, and
for every decision the restatement with that comparison altered is shown to miss a declared output."""
import operator
import os

import numpy as np
import pytest

from gmmloc_amd import synth
from oracle import numpy_ref as nr
from tests import gmm_cases as gc
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def exact():
    return gc.load_exact()


def oracle_build(oracle, mean, cov):
    """what the oracle builds, with hgw and plane4 formed from its sqrt_info and axis in the kernel's expression order"""
    h = oracle.gmm_create(mean, cov)
    out = oracle.gmm_get(h)
    oracle.gmm_destroy(h)
    out["hgw"] = gc.hgw_of(out["sqrt_info"])
    out["plane4"] = gc.plane4_of(out["axis"], np.asarray(mean, dtype=np.float64).reshape(-1, 3))
    return out


ALL_BUILD = gc.ALL_BUILD


def test_case_tables_are_complete():
    for cases in (gc.BUILD, gc.GRAPH, gc.KNN):
        names = [c["name"] for c in cases]
        assert len(set(names)) == len(names)
        assert all(c["decision"] and c["side"] for c in cases)
    for c in gc.BUILD:  # R diag(w) R^T was rounded symmetrically; only asym.* is asymmetric
        if np.all(np.isfinite(c["cov"])):
            assert np.array_equal(c["cov"], c["cov"].T) == (not c["name"].startswith("asym")), c["name"]
    for c in gc.KNN:  # lattice means: every squared distance is an exact double
        m = c["mean"][np.isfinite(c["mean"]).all(axis=1)]
        assert np.array_equal(m, np.round(m)) and np.abs(m).max() < 2 ** 20


def test_golden_regenerates_byte_identically(tmp_path):
    pytest.importorskip("mpmath")
    from tools import make_gmm_cases_golden as mk
    p = tmp_path / "again.npz"
    mk.write(str(p))
    assert p.read_bytes() == open(os.path.join(GOLDEN, "gmm_cases_exact.npz"), "rb").read()


def test_oracle_on_build_cases_and_error_figures(oracle, exact, capsys):
    mean, cov = gc.build_map(ALL_BUILD)
    got = oracle_build(oracle, mean, cov)
    worst = gc.check_build(got, exact[0], ALL_BUILD, "oracle")
    with capsys.disabled():
        print("\noracle, worst error per quantity (units of gmm_cases): " +
              ", ".join("%s %.3g (%s)" % (q, v, n) for q, (v, n) in sorted(worst.items())))
    assert set(worst) == set(gc.ORACLE_WORST) - {"nbs_dist"}
    for q, (v, n) in worst.items():
        assert v <= gc.ORACLE_WORST[q], (q, v, n)  # the figures written next to the bounds are upper figures
    # cov_inv and det against the 60-digit values too (they stay bit-equal between oracle and device)
    for i, c in enumerate(gc.BUILD):
        if c["ok"]:
            ex = exact[0][i]
            cond = gc.kappa(ex["w"])
            assert np.abs(got["cov_inv"][i] - ex["inv"]).max() <= 8 * gc.EPS * cond * np.abs(ex["inv"]).max(), c["name"]
            assert abs(got["det"][i] - ex["det"]) <= 8 * gc.EPS * cond * abs(ex["det"]), c["name"]


@pytest.mark.parametrize("K", gc.BUILD_K_EDGES)
def test_oracle_on_block_edge_maps(oracle, K):
    mean, cov, flags = gc.build_edge_map(K)
    assert np.array_equal(oracle_build(oracle, mean, cov)["flags"], flags)


def test_failed_cholesky_leaves_the_neighbours_rows_alone(oracle):
    good = ["cond1e6", "disc"]
    alone = oracle_build(oracle, *gc.build_map(good))
    for bad in ("bad.indef", "bad.singular", "bad.inf", "bad.nan"):
        mixed = oracle_build(oracle, *gc.build_map([good[0], bad, good[1]]))
        for k in ("cov_inv", "det", "scale", "axis", "sqrt_info", "flags", "hgw", "plane4"):
            assert np.array_equal(mixed[k][[0, 2]], alone[k]), (bad, k)
        assert np.isnan(mixed["sqrt_info"][1]).all() and np.isnan(mixed["hgw"][1]).all()


def test_threshold_cases_lie_on_their_declared_side(oracle, exact):
    """A condition, not a measurement: in 60-digit arithmetic on the rounded matrix every threshold case is on its declared
    side, by at least 20x the oracle's own eigenvalue error for that case.  A case that fails this is replaced."""
    mean, cov = gc.build_map(ALL_BUILD)
    got = oracle_build(oracle, mean, cov)
    n = 0
    for i, c in enumerate(gc.BUILD):
        w = exact[0][i]["w"]
        for e, t in c["thresh"]:
            n += 1
            margin = abs(w[e] - t)
            err = abs(got["scale"][i][e] - w[e])
            assert margin >= 20 * err and margin > 0, (c["name"], e, margin, err)
        if c["thresh"]:
            assert gc.flags_of(w) == c["flags"], c["name"]
    assert n >= 28
    for c in gc.GRAPH:
        if c["name"].startswith("thr.") and c["name"] != "thr.equal":
            d = exact[1][c["name"]][0, 1]
            h = oracle.gmm_create(c["mean"], c["cov"])
            _, col, dist = oracle.neighbour_rows(h, 0, 1, thresh=np.inf)
            oracle.gmm_destroy(h)
            assert list(col) == [1]
            margin, err = abs(d - c["thresh"]), abs(dist[0] - d)
            assert margin >= 20 * err and margin > 1e-7, (c["name"], margin, err)
            assert (d < c["thresh"]) == (c["rows"] == [[1], [0]]), c["name"]


def _oracle_graph(oracle, c):
    h = oracle.gmm_create(c["mean"], c["cov"])
    ptr, col, dist = oracle.neighbours(h, c["thresh"])
    oracle.gmm_destroy(h)
    return ptr, col, dist


def test_oracle_on_graph_cases(oracle, exact, capsys):
    worst, per = (0.0, ""), []
    for c in gc.GRAPH:
        e = gc.check_graph(c, *_oracle_graph(oracle, c), exact[1][c["name"]], gc.graph_cond(c))
        per.append((c["name"], e))
        worst = max(worst, (e, c["name"]))
    with capsys.disabled():
        print("\noracle, worst nbs_dist error: %.3g units (%s)" % worst)
        print("  per case: " + ", ".join("%s %.3g" % x for x in per))
    assert worst[0] <= gc.ORACLE_WORST["nbs_dist"]
    assert gc.GRAPH_BY_NAME["k1"]["rows"] == [[]]
    assert {len(c["mean"]) % 4 for c in gc.GRAPH} == {0, 1, 2, 3}


def test_numpy_ref_on_the_cases(exact):
    """LAPACK's eigh / inv / cholesky share nothing with the Jacobi and the cofactor inverse: flags, eigenvalues and graphs"""
    for i, c in enumerate(gc.BUILD):
        if not c["ok"]:
            continue  # numpy's inverse and Cholesky raise on these
        r = nr.build_components(c["mean"][None], c["cov"].reshape(1, 9))
        assert (int(r["is_deg"][0]) | 2 * int(r["is_salient"][0])) == c["flags"], c["name"]
        w = exact[0][i]["w"]
        assert np.abs(r["scale"][0] - w).max() <= 64 * gc.EPS * w[2], c["name"]
    for c in gc.GRAPH:
        if c["name"] == "negdet":
            continue  # numpy's inverse raises on the singular mean covariance
        C = c["cov"].reshape(-1, 3, 3)
        rows = nr.neighbour_rows(c["mean"], c["cov"], np.linalg.det(C), range(len(C)), c["thresh"])
        if c["name"] == "thr.equal":
            assert abs(nr.bh(c["mean"][0], C[0], 1.0, c["mean"][1], C[1], 1.0) - 2.0) < 1e-14
            continue  # LAPACK's inverse need not give 2.0 exactly
        assert [list(j) for j, _ in rows] == c["rows"], c["name"]


def test_altered_comparisons_miss_a_declared_output(exact):
    """for every decision: the restatement with that comparison altered disagrees with a declared output, and the unaltered
    one agrees with all of them"""
    B = {c["name"]: (c, exact[0][i]) for i, c in enumerate(gc.BUILD)}

    def build_flags(deg=operator.lt, sal=operator.gt, upper=False, sort=True):
        out = {}
        for n, (c, ex) in B.items():
            if not np.all(np.isfinite(c["cov"])):
                continue
            w = ex["wu"] if upper else ex["w"]
            if not sort and c["axis"] is not None:
                w = np.diag(c["cov"])
            out[n] = gc.flags_of(w, deg, sal)
        return out
    want = {n: c["flags"] for n, (c, _) in B.items() if np.all(np.isfinite(c["cov"]))}
    assert build_flags() == want
    miss = lambda got: sorted(n for n in want if got[n] != want[n])
    assert miss(build_flags(deg=operator.le)) == ["diag.at", "diag.sal"]
    assert miss(build_flags(sal=operator.ge)) == ["diag.at", "diag.deg"]
    assert miss(build_flags(upper=True)) == ["asym.lower", "asym.saved", "asym2.lower", "asym2.saved"]
    assert set(miss(build_flags(sort=False))) >= {"order.102", "order.120", "order.201", "order.210", "bad.indef", "bad.singular"}
    # the columns of axis: without the column swap the declared axis of every order but the sorted one is missed
    assert sum(not np.array_equal(c["axis"], np.eye(3)) for c in gc.BUILD if c["name"].startswith("order.")) == 5

    def graphs(lt=operator.lt, skip_self=True):
        out = {}
        for c in gc.GRAPH:
            D = exact[1][c["name"]].copy()
            np.fill_diagonal(D, 0.0)  # a component against itself: the same covariance, no offset
            out[c["name"]] = gc.graph_rule(D, c["thresh"], lt, skip_self)
        return out
    gwant = {c["name"]: c["rows"] for c in gc.GRAPH}
    assert graphs() == gwant
    assert sorted(n for n, r in graphs(lt=operator.le).items() if r != gwant[n]) == ["thr.equal"]
    assert all(r != gwant[n] for n, r in graphs(skip_self=False).items())

    def knn(**kw):
        return {(c["name"], k): gc.knn_rule(c["mean"], c["q"], k, **kw)[0] for c in gc.KNN for k in c["want"]}
    kwant = {(c["name"], k): v for c in gc.KNN for k, v in c["want"].items()}
    assert knn() == kwant
    rev = knn(before=operator.le)  # insert BEFORE the equal ones: highest index first
    assert {n for (n, k), v in rev.items() if v != kwant[(n, k)]} == {"tie.straddle", "tie.inside", "dup.lanes", "tile.513"}
    # `<=` in the gate alone changes nothing: an entry equal to the k-th is placed after it, that is nowhere.  Declared
    # equivalent; the kernels' tie order is held by the placement comparison above.
    assert knn(accept=operator.le) == kwant


def test_oracle_on_knn_cases(oracle):
    for c in gc.KNN:
        if c["name"].startswith("nan."):
            continue  # like KNNResultSet::addPoint the oracle appends a NaN distance where it stands; the device never accepts one
        h = oracle.gmm_create(c["mean"], np.tile(gc.I3, (len(c["mean"]), 1)))
        for k, want in c["want"].items():
            idx, dist, cnt = oracle.knn3d(h, c["q"][None], k)
            wd = np.array(gc.knn_rule(c["mean"], c["q"], k)[1])
            assert list(idx[0]) == want, (c["name"], k, idx[0])
            n = int(cnt[0])
            assert n == sum(i >= 0 for i in want) and np.array_equal(dist[0, :n], wd[:n])  # the oracle leaves the padded distances alone
        oracle.gmm_destroy(h)


def test_live_nanoflann_on_knn_cases(oracle, capsys):
    """The reference's own nanoflann: the same distances everywhere; the same index set wherever no tie straddles the k-th
    place; its order on exact ties is its tree's, not the index order - the declared deviation, recorded here."""
    if oracle.nf is None:
        pytest.skip("oracle/_ref/libnanoflann_ref.so not built")
    differs = []
    for c in gc.KNN:
        if not np.isfinite(c["mean"]).all() or not np.isfinite(c["q"]).all():
            continue  # a kd-tree over NaN has no defined behaviour
        d0 = c["q"][None] - c["mean"]
        alld = np.sort((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2])
        for k, want in c["want"].items():
            idx, dist, cnt = oracle.nanoflann_knn(c["mean"], c["q"][None], k)
            n = int(cnt[0])
            wd = np.array(gc.knn_rule(c["mean"], c["q"], k)[1])
            assert n == min(k, len(c["mean"])) and np.array_equal(dist[0, :n], wd[:n]), (c["name"], k)
            straddle = len(alld) > k and alld[k - 1] == alld[k]
            if not straddle:
                assert sorted(idx[0, :n]) == sorted(want[:n]), (c["name"], k)
            if list(idx[0, :n]) != want[:n]:
                differs.append((c["name"], k, list(idx[0, :n]), want[:n], bool(straddle)))
    with capsys.disabled():
        print("\nnanoflann's order differs from lowest-index-first on %d (case, k), in %d of them as a set; at k = 8:"
              % (len(differs), sum(sorted(d[2]) != sorted(d[3]) for d in differs)))
        for d in differs:
            if d[1] == 8:
                print("  %s nanoflann %s declared %s" % (d[0], [int(x) for x in d[2]], d[3]))
    got = {k: v for n, k, v, _, _ in differs if n == "tie.straddle"}
    assert all(got.get(k) == v for k, v in gc.NANOFLANN_OCTA.items()), got
    assert all(d[0].startswith(("tie.", "dup.", "tile.513")) for d in differs)  # only where there are exact ties


@pytest.mark.parametrize("which", ["v1", "v2"])
def test_the_tie_deviation_touches_nothing_shipped(map_v1, map_v2, which):
    """no two means of the shipped maps are equal, and the recorded golden queries have no exact tie among their six nearest"""
    mean, cov = {"v1": map_v1, "v2": map_v2}[which]
    assert len(np.unique(mean, axis=0)) == len(mean)
    pts = synth.synth_points(mean, cov, 1500, 9)  # the queries of golden_nanoflann_knn.npz
    for lo in range(0, len(pts), 250):
        d = pts[lo:lo + 250, None, :] - mean[None, :, :]
        d2 = np.sort((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)[:, :6]
        assert (np.diff(d2, axis=1) > 0).all()
