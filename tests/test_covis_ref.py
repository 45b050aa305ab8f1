"""CPU: tests/covis_ref.py held to the declarations of tests/covis_cases.py - the sequential object model and the numpy statement of
the row representation, each against every hand-written output - and the fact the layout of gl_map_covis rests on: over random edit
sequences the model's ordered list is ALWAYS the prefix of its row in the declared order (Model.rows asserts it), so the prefix length
loses nothing; the two statements agree after every step."""
import copy

import numpy as np
import pytest

from tests import covis_cases as CC
from tests import covis_ref as R

ENTRY_POINTS = ("gl_covis_update", "gl_covis_remove", "gl_covis_best", "gl_fuse_targets", "gl_fuse_candidates")
# the cases whose input no sequence of the reference's calls produces (capacity, rows outside a table): the numpy statement only
ROWS_ONLY = {"w_truncated", "rows_outside_the_table", "kf2_skipped", "cap_below", "conn_cap_below"}


def test_entry_points_are_bound():
    from gmmloc_amd import _lib
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in lib._gl_signatures, name


def _update_inputs(c):
    m = CC.shared_map(c["shared"], c.get("invalid_kf", ()), c.get("invalid_shared"))
    return m, CC.graph(CC.NKF, c["Wcap"], c["rows0"], c.get("best0"))


@pytest.mark.parametrize("name", list(CC.UPDATE))
def test_update_rows(name):
    c = CC.UPDATE[name]
    m, g = _update_inputs(c)
    g0 = copy.deepcopy(g)
    out = R.rows_update(g, m, 0, c["Ccap"])
    CC.assert_graph(g, g0, c["out"]["rows"], c.get("best0", {}), name)
    CC.assert_list(out["conn_kf"], [k for k, _ in c["out"]["conn"]], name)
    CC.assert_list(out["conn_w"], [w for _, w in c["out"]["conn"]], name)
    assert out["n_conn"].tolist() == [c["out"]["n_conn"]] and out["result"].tolist() == c["out"]["result"], (name, out)


@pytest.mark.parametrize("name", [n for n in CC.UPDATE if n not in ROWS_ONLY])
def test_update_model(name):
    c = CC.UPDATE[name]
    m, g0 = _update_inputs(c)
    md = R.Model.from_rows(g0)
    status = md.update_connections(m, 0)
    assert status == c["out"]["result"][1], name
    CC.assert_graph(md.rows(c["Wcap"]), g0, c["out"]["rows"], c.get("best0", {}), name)
    k = md.kfs[0]
    if not status:
        assert list(zip(k.ordered, k.ordered_w)) == c["out"]["conn"] and len(k.ordered) == c["out"]["n_conn"], name


@pytest.mark.parametrize("name", list(CC.REMOVE))
def test_remove_rows(name):
    c = CC.REMOVE[name]
    g = CC.graph(CC.NKF, 4, c["rows0"], c["best0"])
    g0 = copy.deepcopy(g)
    res = R.rows_remove(g, CC.NKF, c["list"][:c.get("n_cull", len(c["list"]))], c["kf_first"])
    CC.assert_graph(g, g0, c["out"]["rows"], c["out"]["best"], name)
    assert res.tolist() == c["out"]["result"], (name, res)


@pytest.mark.parametrize("name", [n for n in CC.REMOVE if n not in ROWS_ONLY])
def test_remove_model(name):
    c = CC.REMOVE[name]
    g0 = CC.graph(CC.NKF, 4, c["rows0"], c["best0"])
    md = R.Model.from_rows(g0)
    tot = [0, 0, 0]
    for r in c["list"][:c.get("n_cull", len(c["list"]))]:
        rm, er, st = md.remove_key_frame(r, c["kf_first"])
        tot = [tot[0] + rm, tot[1] | st, tot[2] + er]
    CC.assert_graph(md.rows(4), g0, c["out"]["rows"], c["out"]["best"], name)
    assert tot + [0] == c["out"]["result"], (name, tot)


@pytest.mark.parametrize("name", list(CC.BEST))
def test_best(name):
    c = CC.BEST[name]
    g = CC.graph(CC.NKF, 4, CC.BEST_ROWS)
    out = R.rows_best(g, CC.NKF, c["kf"], c["N"], c["Ccap"])
    md = R.Model.from_rows(g)
    for b, pairs in enumerate(c["out"]["conn"]):
        CC.assert_list(out["conn_kf"][b], [k for k, _ in pairs], name)
        CC.assert_list(out["conn_w"][b], [w for _, w in pairs], name)
        if 0 <= c["kf"][b] < CC.NKF and c["out"]["n_conn"][b] <= c["Ccap"]:
            assert [list(v) for v in md.best_covisibles(c["kf"][b], c["N"])] == [[k for k, _ in pairs], [w for _, w in pairs]], name
    assert out["n_conn"].tolist() == c["out"]["n_conn"] and out["result"].tolist() == c["out"]["result"], (name, out)


@pytest.mark.parametrize("name", list(CC.TARGETS))
def test_targets(name):
    c = CC.TARGETS[name]
    g = CC.graph(c["nkf"], 12, c["rows"])
    valid = np.ones(c["nkf"], np.uint8)
    valid[list(c.get("invalid_kf", ()))] = 0
    out = R.rows_targets(g, c["nkf"], valid, 0, c["nn"], c["nn2"], c["Tcap"])
    CC.assert_list(out["tgt_kf"], c["out"]["tgt"], name)
    assert out["n_tgt"].tolist() == [c["out"]["n_tgt"]] and out["result"].tolist() == c["out"]["result"], (name, out)
    if name not in ROWS_ONLY:
        tgt = R.Model.from_rows(g).fuse_targets(0, valid, c["nn"], c["nn2"])
        assert tgt[:c["Tcap"]] == c["out"]["tgt"] and len(tgt) == c["out"]["n_tgt"], (name, tgt)


@pytest.mark.parametrize("name", list(CC.CANDIDATES))
def test_candidates(name):
    c = CC.CANDIDATES[name]
    m = CC.cand_map()
    out = R.rows_candidates(m, np.array(c["tgt"], np.int32), c["n_tgt"], c["kf_idx"], c["cand_cap"])
    CC.assert_list(out["cand_mp"], c["out"]["cand"], name)
    assert out["n_cand"].tolist() == [c["out"]["n_cand"]] and out["result"].tolist() == c["out"]["result"], (name, out)
    seq = R.fuse_candidates(m, c["tgt"][:c["n_tgt"]], c["kf_idx"])
    assert seq[:c["cand_cap"]] == c["out"]["cand"] and len(seq) == c["out"]["n_cand"], (name, seq)


def apply_step(step, m, md, g, Ccap=64):
    """one edit of CC.random_steps on the map, the model (may be None) and the rows -> what the rows' call returned"""
    if step[0] == "flip":
        m["mp_valid"][step[1]] ^= 1
        return None
    if step[0] == "update":
        if md is not None:
            md.update_connections(m, step[1])
        return R.rows_update(g, m, step[1], Ccap)
    if md is not None:
        for r in step[1]:
            md.remove_key_frame(r, step[2])
    return R.rows_remove(g, CC.R_NKF, step[1], step[2])


@pytest.mark.parametrize("seed", [3, 4])
def test_random_edit_sequences_keep_the_prefix(seed):
    m = CC.random_map(seed)
    W = CC.R_NKF
    md, g = R.Model(CC.R_NKF), CC.graph(CC.R_NKF, W, {})
    seen = dict(changed=0, same=0, below=0, whole=0, removed=0)
    for i, step in enumerate(CC.random_steps(seed + 100, 300)):
        before = g["cov_nord"].copy()
        out = apply_step(step, m, md, g)
        ref = md.rows(W)  # asserts the prefix invariant on every row
        for k in range(CC.R_NKF):
            n = int(ref["cov_n"][k])
            assert (n, int(ref["cov_nord"][k]), int(ref["best_cov"][k])) == (int(g["cov_n"][k]), int(g["cov_nord"][k]), int(g["best_cov"][k])), (i, step, k)
            assert np.array_equal(ref["cov_kf"][k, :n], g["cov_kf"][k, :n]) and np.array_equal(ref["cov_w"][k, :n], g["cov_w"][k, :n]), (i, step, k)
        if step[0] == "update":
            seen["changed"] += int(out["result"][2])
            seen["same"] += int(out["n_conn"][0]) - int(out["result"][2])
            seen["below"] += int((g["cov_w"][step[1], :g["cov_n"][step[1]]] < R.TH).any())
            seen["whole"] += int(((g["cov_nord"] == g["cov_n"]) & (g["cov_nord"] > before) & (g["cov_n"] > 1)).any())
        elif step[0] == "remove":
            seen["removed"] += int(out[0])
        if i % 20 == 0:
            kf = int(np.argmax(g["cov_nord"]))
            t = R.rows_targets(g, CC.R_NKF, m["kf_valid"], kf, 10, 5, 60)
            assert md.fuse_targets(kf, m["kf_valid"]) == t["tgt_kf"][:int(t["n_tgt"][0])].tolist(), (i, kf)
    assert all(v > 5 for v in seen.values()), seen  # every branch was walked: the test does not pass vacuously
