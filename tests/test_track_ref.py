"""tests/track_ref.py (Tracking::track up to trackLocalMap, restated from the reference's text) on the frames of tests/track_cases.py:
every case hits the counts it declares, every branch of tracking.cpp:53, :65, :345 and :352 is taken with its operand on BOTH sides
of the threshold, the below-20 cases tell the reference's early return (:352) from "optimise anyway", and the host glue of the
device tests (tests/chain_glue.py) equals the model on every case.  CPU only."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import chain_glue as G
from tests import track_cases as TC
from tests import track_ref as T

CAM = api.Camera()
LAYOUTS = [(n, True) for n in TC.CASES] + [(n, False) for n in TC.NO_FALLBACK]


@pytest.fixture(scope="module")
def results(oracle):
    """the model's result of every case in both buffer layouts, computed once"""
    return {(n, fb): T.track(oracle, CAM, TC.frame(oracle, n, fb)) for n, fb in LAYOUTS}


class OptimiseAnyway(T.Tracking):
    """what the chain did before it followed :352: the optimisation and the outlier loop (:356-373) run on a frame of fewer than 20
    matches all the same, and only the return value is zeroed"""

    def track_with_motion_model(self):
        ret = super().track_with_motion_model()
        if self.n1 < 20:
            fr = self.frame
            self.optimize_current_pose()
            for i in range(self.NF):
                mp = fr.mappoints[i]
                if mp is not None and fr.is_outlier[i]:
                    fr.mappoints[i], fr.is_outlier[i] = None, False
                    mp.cell.last_visible_idx = fr.idx
                    self.drop_src[i] = mp.k
        return ret


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_hits_its_declared_counts(results, name):
    r, want = results[(name, True)], TC.CASES[name][1]
    for k, v in want.items():
        if k == "n1_min":
            assert r["n1"] >= v, (name, k, r["n1"])
        else:
            assert r[k] == v, (name, k, r[k])
    if name in TC.NO_FALLBACK:  # without the key-frame's buffers: the same trackWithMotionModel, never the fallback
        q = results[(name, False)]
        assert (q["n1"], q["ret_mm"]) == (r["n1"], r["ret_mm"]) and q["mode"] == 0 and q["nbow"] == 0 and (q["match_kf"] == -1).all()


def test_every_branch_is_taken_on_both_sides_of_its_threshold(results):
    rs = [r for (n, fb), r in results.items() if fb]
    n7 = {r["n7"] for r in rs}
    n1 = {r["n1"] for r in rs}
    ret_mm = {r["ret_mm"] for r in rs if r["n1"] >= 20}
    ret_kf = {r["ret_kf"] for r in rs if r["mode"] != 0}
    nbow = {r["nbow"] for r in rs if r["mode"] != 0}
    assert {19, 20} <= n7                  # tracking.cpp:345
    assert {9, 10, 19, 20} <= n1           # tracking.cpp:352
    assert {9, 10} <= ret_mm               # tracking.cpp:53 (with 20 matches or more: the value is a count, not :353's false)
    assert {9, 10} <= ret_kf               # tracking.cpp:65
    assert {14, 15} <= nbow                # tracking.cpp:305
    assert any(r["retried"] and r["n1"] >= 20 for r in rs) and any(r["retried"] and r["n1"] < 20 for r in rs)
    assert {r["mode"] for r in rs} == {0, 1, 2}
    # :53 is reached from :353 and from :376
    assert any(r["mode"] == 1 and r["n1"] < 20 for r in rs) and any(r["mode"] == 1 and r["n1"] >= 20 for r in rs)


def test_nbow_14_and_15_take_the_same_path(results):
    """:305 only logs: the frames either side of it are tracked through the key-frame alike"""
    a, b = results[("nbow_14", True)], results[("nbow_15", True)]
    assert (a["nbow"], b["nbow"]) == (14, 15) and a["mode"] == b["mode"] == 1
    assert a["ret_kf"] + (a["drop_kf"] >= 0).sum() == 14 and b["ret_kf"] + (b["drop_kf"] >= 0).sum() == 15
    assert a["n3"] > 0 and b["n3"] > 0


def test_below_20_cases_tell_the_early_return_from_optimise_anyway(oracle, results):
    """the cases would catch a chain that optimises a frame of fewer than 20 matches: its outliers are dropped and marked seen, so
    with the fallback searchLocalPoints sees other candidates, and without it the pose and the matches are not stage 1's"""
    small = [n for n in TC.BELOW_20 if n not in TC.LARGE]
    assert len(small) >= 7
    differ_m3 = 0
    for n in small:
        r = results[(n, True)]
        a = OptimiseAnyway(oracle, CAM, TC.frame(oracle, n)).track()
        assert (r["drop_src"] == -1).all() and (a["drop_src"] >= 0).sum() >= 1, n
        assert not np.array_equal(r["seen"], a["seen"]), n
        differ_m3 += int(not np.array_equal(r["match_local"], a["match_local"]))
    assert differ_m3 >= 2
    for n in [n for n in small if n in TC.NO_FALLBACK]:
        f = TC.frame(oracle, n, False)
        r = results[(n, False)]
        a = OptimiseAnyway(oracle, CAM, f).track()
        assert np.array_equal(r["pose"], f["pose_cw"]) and r["ninl"] == 0 and (r["match_last"] >= 0).sum() == r["n1"], n
        assert np.abs(a["pose"] - f["pose_cw"]).max() > 1e-3 and (a["match_last"] >= 0).sum() < r["n1"], n


@pytest.mark.parametrize("name,fallback", LAYOUTS)
def test_chain_glue_equals_the_model(oracle, results, name, fallback):
    """tests/chain_glue.py says the same thing in array expressions: every decision, list and the stage-2 pose (the same oracle calls:
    the same bits), and searchLocalPoints from that pose"""
    f, r = TC.frame(oracle, name, fallback), results[(name, fallback)]
    g = G.oracle_front(oracle, CAM, f)
    for k in ("n1", "ret_mm", "nbow", "ret_kf", "mode", "ninl"):
        assert g[k] == r[k], k
    for k in ("match_last", "match_kf", "drop_src", "drop_kf", "pose"):
        assert np.array_equal(g[k], r[k]), k
    if r["mode"] == 2:
        return
    m3, n3, iv = G.oracle_stage3(oracle, CAM, f, g["pose"], g["match_last"], g["match_kf"], g["drop_src"], g["drop_kf"])
    assert n3 == r["n3"] and np.array_equal(m3, r["match_local"]) and np.array_equal(iv, r["inview"])
    Xg = G.pose_inputs(f, g["match_last"], m3, g["match_kf"])
    Xr = T.pose_problem(f, r)
    assert all(np.array_equal(a, b) for a, b in zip(Xg, Xr))
