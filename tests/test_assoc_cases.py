"""CPU: the hand-built association cases (tests/assoc_cases.py) against the bit-exact host model (tests/assoc_model.py), rational
arithmetic and the C++ oracle.

  * the model IS the arithmetic: its records and its chi2 equal the oracle's bits on every case (the device is held to both in
    tests/test_gpu_assoc_cases.py);
  * am.admitted() - build_cell_index's host predicate, read off the source - gives the `always` every admit.* case declares, and the
    declared winners are the model's;
  * non-vacuity: the gate.tip scans hold points the index can lose (counts below);
  * THE MARGIN: for every component the index registers, |computed chi2 / exact chi2 - 1| at the gate stays below what its
    registration leaves, (1 + 4e-6) / (1 + 1e-6) - 1 - 2e-9 = 2.998e-6 for every component whose error bound is below that (every
    component of the EuRoC maps' planes and of the synthetic maps), with all figures read from gl_grid.hip.

Measured with this model, worst of 200 rotations at the six tips of the gate ellipsoid (error_table() prints it again; DESIGN.md
section 4 has it too):
    condition       1e2      1e4      1e5      8e5      1e6      1e7      3e7      9.9e7
    plane         1.1e-14  1.1e-12  1.1e-11  7.1e-11  9.7e-11  1.0e-9   3.0e-9   8.7e-9
    general       1.1e-14  1.4e-11  5.3e-10  7.2e-9   1.1e-8   4.8e-7   2.9e-6   1.4e-5
    needle        1.0e-13  7.0e-10  1.0e-7   6.0e-6   7.4e-6   1.0e-3   1.0e-2   8.5e-2
so with the condition number <= 1e8 as the only admission rule the needles from 8e5 on and general ellipsoids near 1e8 break the
2.998e-6 the plain registration leaves.
"""
import math

import numpy as np
import pytest

from tests import assoc_cases as ac
from tests import assoc_model as am

Fr = am.Fr
FAMILIES = {"plane": lambda k: (1e-6, 0.7e-6 * k, 1e-6 * k), "general": lambda k: (0.16 / k, 0.16 / math.sqrt(k), 0.16),
            "needle": lambda k: (0.16 / k, 1.3 * 0.16 / k, 0.16)}
CONDS = (1e2, 1e4, 1e5, 8e5, 1e6, 1e7, 3e7, 9.9e7)  # (8e5: the needles registered at a gate of their own, see test_margin_...)


def haar(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))[None, :]


def gate_error(mean, cov):
    """the worst |computed / exact - 1| of chi2 over the six tips of the gate ellipsoid (its principal axes by numpy)"""
    w, V = np.linalg.eigh(cov)
    rec, worst = am.record(mean, cov), 0.0
    for a in range(3):
        for sgn in (1.0, -1.0):
            p = mean + sgn * math.sqrt(am.T_GATE * w[a]) * V[:, a]
            worst = max(worst, abs(float(Fr(am.chi2_device(rec, p)) / am.chi2_exact(cov, mean, p) - 1)))
    return worst


def random_components(family, cond, n=200):
    rng = np.random.default_rng([int(cond), len(family)])
    for _ in range(n):
        yield ac.comp(rng.uniform(-3, 3, 3), FAMILIES[family](cond), haar(rng))


def error_table():
    for fam in FAMILIES:
        print(fam, " ".join("%.1e" % max(gate_error(*c) for c in random_components(fam, k)) for k in CONDS))


def test_model_is_the_oracles_arithmetic(oracle):
    """records, argmin and chi2 of the model equal the C++ oracle's by the bits on every case"""
    for c in ac.CASES.values():
        h = oracle.gmm_create(c.mean, c.cov.reshape(-1, 9))
        try:
            inv = oracle.gmm_get(h)["cov_inv"].reshape(-1, 9)
            with np.errstate(all="ignore"):
                idx, d2 = oracle.associate3d(h, c.pts)
        finally:
            oracle.gmm_destroy(h)
        for k in sorted(set(c.under) | {0, c.K - 1}):
            assert np.array_equal(inv[k], np.array(am.record(c.mean[k], c.cov[k])[3:]), equal_nan=True), (c, k)
        m = c.model()
        assert np.array_equal(idx, m["idx"]) and np.array_equal(d2, m["d2"]), c


def test_declared_winners_are_the_models():
    n = 0
    for c in ac.CASES.values():
        said = c.winner >= 0
        assert np.array_equal(c.model()["idx"][said], c.winner[said]), c
        n += int(said.sum())
    assert n > 100


def test_admitted_gives_the_declared_always():
    sides = set()
    for c in ac.CASES.values():
        if c.always is None:
            continue
        adm = [am.admitted(m, cv) for m, cv in zip(c.mean, c.cov)]
        assert sum(a is False for a in adm) + c.by_box == c.always, (c, c.always)
        if c.name.startswith("admit."):
            sides.add((c.name, adm[0]))
    want = {("admit.plane_below_cond", True), ("admit.plane_above_cond", False), ("admit.needle_below_cond", False),
            ("admit.needle_above_cond", False), ("admit.needle_below_err", True), ("admit.needle_above_err", False),
            ("admit.needle_below_slack", True), ("admit.needle_above_slack", True), ("admit.asym_below", True), ("admit.asym_above", False), ("admit.nonfinite", None), ("admit.singular", False),
            ("admit.indefinite", False), ("admit.box", True), ("admit.box_default", True)}
    assert sides == want, sides ^ want
    # the sides are sides: each pair straddles ITS limit and no other
    k = am.source_constants()
    for name, lam_cond in (("admit.plane_below_cond", 9.9e7), ("admit.plane_above_cond", 1.01e8)):
        w = am.eig3_sym(list(map(float, ac.CASES[name].cov[0].reshape(9))))
        assert abs(w[2] / w[0] / lam_cond - 1) < 1e-6 and am.gate_error_bound(w) < k["slack"], name
    for name, f in (("admit.needle_below_err", 0.99), ("admit.needle_above_err", 1.01)):
        w = am.eig3_sym(list(map(float, ac.CASES[name].cov[0].reshape(9))))
        assert abs(am.gate_error_bound(w) / (f * k["err_max"]) - 1) < 1e-6 and w[2] / w[0] < k["cond"], name


def test_tip_scans_hold_what_the_index_can_lose():
    """Non-vacuity, by the model: over the gate.tip scans at least 8 points with chi2(needle) < chi2(second) <= 9 (1 + 1e-6) as computed,
    and at least 8 whose computed chi2 is <= 9 (1 + 1e-6) while the exact one is above 9 (1 + 4e-6), the plain
    registration gate.  Counted: 0 / 0 / 4 / 30 / 1 640 lost points of 4 096 at condition 1e4 / 1e6 / 1e7 / 3e7 / 9.9e7 (820 in between at each)."""
    lost, between = {}, {}
    for n in ac.names("gate.tip"):
        s = ac.tip_sets(ac.CASES[n])
        lost[n], between[n] = int(s["lost"].sum()), int(s["between"].sum())
    print("lost", lost, "between", between)
    assert sum(between.values()) >= 8 and sum(lost.values()) >= 8
    assert lost["gate.tip.1e+04"] == 0  # ... and none on the needle the index still registers
    for n in ac.names("gate.tip"):
        assert len(ac.track_points(ac.CASES[n])) >= 8


def test_the_widened_gate_is_needed_and_is_the_sources():
    """The one decision of the registration that is not an admission: a component whose error bound exceeds the slack is registered at
    9 (1 + 4e-6) / (1 - bound).  One needle on either side of it (bound = 0.99 / 1.01 of the slack); and gate.wide, the needle of
    condition 8e5 whose computed chi2 is 6.7e-6 low: by the model 274 of its 4 096 scan points are resolved while their exact chi2 is above
    9 (1 + 4e-6) - without the wider gate they are outside what is registered -, none is above the gate it IS registered at.  The model
    takes the wider gate from the statements of gl_grid.hip, so without them this test and the margin test fail."""
    k = am.source_constants()
    assert k["widen"] and k["widen_used"]
    below, above = (ac.CASES["admit.needle_%s_slack" % s].cov[0] for s in ("below", "above"))
    for cv, f in ((below, 0.99), (above, 1.01)):
        assert abs(am.gate_error_bound(am.eig3_sym(list(map(float, cv.reshape(9))))) / (f * k["slack"]) - 1) < 1e-6
    assert am.registered_gate(below) == 1.0 + k["reg"] and am.slack_of(below) == k["slack"]
    assert am.registered_gate(above) == (1.0 + k["reg"]) / (1.0 - am.gate_error_bound(am.eig3_sym(list(map(float, above.reshape(9))))))
    c = ac.CASES["gate.wide.8e+05"]
    assert am.admitted(c.mean[0], c.cov[0]) and am.slack_of(c.cov[0]) > 100 * k["slack"]
    s = ac.tip_sets(c)
    print("gate.wide lost at the plain gate", int(s["lost"].sum()), "at its own", int(s["lost_own"].sum()), "between", int(s["between"].sum()))
    assert s["lost"][:2048].sum() >= 8 and s["lost"][2048:].sum() >= 8 and s["between"].sum() >= 8
    assert s["lost_own"].sum() == 0
    assert gate_error(c.mean[0], c.cov[0]) > 2 * k["slack"]
    assert len(set(ac.track_points(c)) & set(np.nonzero(s["lost"])[0])) >= 8


def test_edge_cases_sit_inside_their_margins():
    """edge.wide / edge.plain (the geometry - cell boundary, box ends, the fillers' corners - is asserted where they are built): at point 0
    chi2(component) < chi2(second) <= 9 (1 + 1e-6) as computed, so an index that does not list the component in that cell answers with the
    second one.  edge.wide: computed below 9 (gl_track_frames keeps it), exact above 9 (1 + 4e-6) - only the gate of its own covers it.
    edge.plain: exact in (9, 9 (1 + 1e-6)] - only the inflation of the registration gate covers it."""
    for name in ("edge.wide", "edge.plain"):
        c = ac.CASES[name]
        p = c.pts[0]
        d0, d1 = (am.chi2_device(am.record(c.mean[k], c.cov[k]), p) for k in (0, 1))
        ex = am.chi2_exact(c.cov[0], c.mean[0], p)
        assert d0 < d1 <= ac.T_RESOLVE and am.admitted(c.mean[0], c.cov[0]), name
        if name == "edge.wide":
            assert d0 <= 9.0 and Fr(ac.T_REG) < ex < Fr(9.0) * Fr(am.registered_gate(c.cov[0]))
        else:
            assert d0 > 9.0 and Fr(9.0) < ex <= Fr(ac.T_RESOLVE) and am.registered_gate(c.cov[0]) == 1.0 + am.source_constants()["reg"]


def check_margin(mean, cov, what):
    k = am.source_constants()
    w = am.eig3_sym(list(map(float, np.asarray(cov).reshape(9))))
    bound, slack, err = am.gate_error_bound(w), am.slack_of(cov), gate_error(mean, cov)
    if bound <= k["slack"]:  # registered at T (1 + 4e-6) like every component before: the slack is the source's plain figure
        assert slack == k["slack"], what
    assert 0 < k["slack"] < 3e-6 and slack >= k["slack"]
    assert err < slack, (what, err, slack)
    assert err <= bound, (what, err, bound)  # the bound build_cell_index decides on is one
    return err


def test_margin_on_every_admitted_component():
    """|chi2_device / chi2_exact - 1| at the gate < the slack gl_grid.hip leaves, for every component of every case that it registers
    and for 200 seeded rotations per shape family and condition number."""
    seen, n = set(), 0
    for c in ac.CASES.values():
        for m, cv in zip(c.mean, c.cov):
            key = cv.tobytes()
            if key in seen or not am.admitted(m, cv):
                continue
            seen.add(key)
            check_margin(m, cv, c.name)
            n += 1
    assert n >= 12
    worst = {}
    for fam in FAMILIES:
        for cond in CONDS:
            errs = [check_margin(m, cv, (fam, cond)) for m, cv in random_components(fam, cond) if am.admitted(m, cv)]
            worst[fam, cond] = (len(errs), max(errs, default=0.0))
    print(worst)
    assert all(worst["plane", k][0] == 200 for k in CONDS)            # what the maps are made of stays in the grid ...
    assert worst["needle", 1e4][0] == 200 and worst["needle", 1e6][0] == 0  # ... and the needles leave it where they must
    # in between they are registered at a gate of their own, and need it: the plain slack would not hold their error
    assert worst["needle", 8e5][0] == 200 and worst["needle", 8e5][1] > am.source_constants()["slack"]


def test_track_scenes_keep_their_association(oracle):
    """What the GPU test relies on: through jointOptimization with one free pose (the oracle) the point on a scan point keeps the
    argmin gated at 9 - no association is dropped by the refinement."""
    from tests import optim_cases as oc
    for c in ac.CASES.values():
        if not c.track:
            continue
        for n in ac.track_points(c)[::5]:
            d = ac.track_scene(c, n)
            idx, d2 = oc.associate(oracle, d["mean"], d["cov"], d["Xw"])
            assert idx[ac.TRACK_SLOT] == c.model()["idx"][n] and d2[ac.TRACK_SLOT] == c.model()["d2"][n]
            assert np.array_equal(oc.run(oracle, "track", d)["assoc"], np.where(d2 <= 9.0, idx, -1)), (c, n)
