"""Every declared case of tests/covis_cases.py on the device: gl_covis_update, gl_covis_remove, gl_covis_best, gl_fuse_targets and
gl_fuse_candidates give the hand-written outputs exactly.  Guard words stand behind every array a call may write, the tables are filled
with a sentinel beyond each row's cov_n (a word behind a row's longer length must still hold it), and every output starts as zeros."""
import copy

import numpy as np
import pytest

from tests import covis_cases as CC
from tests import covis_dev as D
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CC.UPDATE))
def test_update(gpu, name):
    torch, ctx = gpu
    c = CC.UPDATE[name]
    m = CC.shared_map(c["shared"], c.get("invalid_kf", ()), c.get("invalid_shared"))
    g0 = CC.graph(CC.NKF, c["Wcap"], c["rows0"], c.get("best0"))
    dg = D.DevGraph(torch, copy.deepcopy(g0))
    out = D.d_update(torch, ctx, D.dev_map(torch, m), dg, 0, c["Ccap"])
    g = dg.host()
    if c["out"]["result"][1] & CC.W_TRUNCATED:  # the refusal leaves every byte of the graph as it was
        assert all(np.array_equal(g[k], g0[k]) for k in g0), name
    CC.assert_graph(g, g0, c["out"]["rows"], c.get("best0", {}), name)
    CC.assert_list(out["conn_kf"], [k for k, _ in c["out"]["conn"]], name)
    CC.assert_list(out["conn_w"], [w for _, w in c["out"]["conn"]], name)
    assert out["n_conn"].tolist() == [c["out"]["n_conn"]] and out["result"].tolist() == c["out"]["result"], (name, out)


@pytest.mark.parametrize("name", list(CC.REMOVE))
def test_remove(gpu, name):
    torch, ctx = gpu
    c = CC.REMOVE[name]
    g0 = CC.graph(CC.NKF, 4, c["rows0"], c["best0"])
    dg = D.DevGraph(torch, copy.deepcopy(g0))
    res = D.d_remove(torch, ctx, dg, CC.NKF, c["list"], c["kf_first"], c.get("n_cull"))
    CC.assert_graph(dg.host(), g0, c["out"]["rows"], c["out"]["best"], name)
    assert res.tolist() == c["out"]["result"], (name, res)


@pytest.mark.parametrize("name", list(CC.BEST))
def test_best(gpu, name):
    torch, ctx = gpu
    c = CC.BEST[name]
    g0 = CC.graph(CC.NKF, 4, CC.BEST_ROWS)
    dg = D.DevGraph(torch, copy.deepcopy(g0))
    out = D.d_best(torch, ctx, dg, CC.NKF, c["kf"], c["N"], c["Ccap"])
    g = dg.host()
    assert all(np.array_equal(g[k], g0[k]) for k in g0), (name, "a reader wrote the graph")
    for b, pairs in enumerate(c["out"]["conn"]):
        CC.assert_list(out["conn_kf"][b], [k for k, _ in pairs], name)
        CC.assert_list(out["conn_w"][b], [w for _, w in pairs], name)
    assert out["n_conn"].tolist() == c["out"]["n_conn"] and out["result"].tolist() == c["out"]["result"], (name, out)


@pytest.mark.parametrize("name", list(CC.TARGETS))
def test_targets(gpu, name):
    torch, ctx = gpu
    c = CC.TARGETS[name]
    g0 = CC.graph(c["nkf"], 12, c["rows"])
    dg = D.DevGraph(torch, copy.deepcopy(g0))
    valid = np.ones(c["nkf"], np.uint8)
    valid[list(c.get("invalid_kf", ()))] = 0
    out = D.d_targets(torch, ctx, dg, c["nkf"], valid, 0, c["nn"], c["nn2"], c["Tcap"])
    g = dg.host()
    assert all(np.array_equal(g[k], g0[k]) for k in g0), (name, "a reader wrote the graph")
    CC.assert_list(out["tgt_kf"], c["out"]["tgt"], name)
    assert out["n_tgt"].tolist() == [c["out"]["n_tgt"]] and out["result"].tolist() == c["out"]["result"], (name, out)


def test_targets_without_a_valid_array(gpu):
    """kf_valid NULL: every key-frame is valid, the invalid_kf1 case loses its skip"""
    torch, ctx = gpu
    c = CC.TARGETS["invalid_kf1"]
    out = D.d_targets(torch, ctx, D.DevGraph(torch, CC.graph(c["nkf"], 12, c["rows"])), c["nkf"], None, 0, c["nn"], c["nn2"], c["Tcap"])
    CC.assert_list(out["tgt_kf"], [1, 3, 2, 4])
    assert out["n_tgt"].tolist() == [4]


@pytest.mark.parametrize("name", list(CC.CANDIDATES))
def test_candidates(gpu, name):
    torch, ctx = gpu
    c = CC.CANDIDATES[name]
    out = D.d_candidates(torch, ctx, D.dev_map(torch, CC.cand_map()), c["tgt"], c["n_tgt"], c["kf_idx"], c["cand_cap"])
    CC.assert_list(out["cand_mp"], c["out"]["cand"], name)
    assert out["n_cand"].tolist() == [c["out"]["n_cand"]] and out["result"].tolist() == c["out"]["result"], (name, out)
