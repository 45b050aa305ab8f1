"""The hand-built optimiser cases (tests/optim_cases.py) on the CPU: the C++ oracle and oracle/numpy_ref.py both give the output every case
declares; the cases at a threshold sit in their band; every decision has two sides; every case is STABLE (12 re-orderings of its edges and
36 one-ulp perturbations of its inputs leave every declared integer where it is and move the oracle's pose by less than 1e-6); and the
cases can fail: numpy_ref with one comparison altered (ALTERED below) misses the declared output of at least one case of that decision.
The cases of gl_track_frames_anchored (call "anchored") get the same: their re-orderings permute the point slots and the fixed columns,
every decision that has such cases is held by one of them alone, every one at a threshold bites on its own, and each case converted from
a local-BA case is shown to be that case (the oracle on both forms: equal masks, the pose to 1e-12)."""
import numpy as np
import pytest

from oracle import numpy_ref
from tests import optim_cases as oc
from tests.test_gpu_pose import pose_err
from tests.test_gpu_soak_cases import ulp_variants

F32 = np.float32
NAMES = sorted(oc.CASES)
_memo = {}


def outputs(backend, name):
    key = (backend is numpy_ref, name)
    if key not in _memo:
        c = oc.CASES[name]
        o = oc.run(backend, c.call, c.data, trace=True) if backend is numpy_ref else oc.run(backend, c.call, c.data)
        if backend is numpy_ref and c.call in ("track", "anchored"):
            o["outer"] = sum(len(t["q"]) for t in o["trace"]["lm"])
        _memo[key] = o
    return _memo[key]


@pytest.mark.parametrize("name", NAMES)
def test_case_gives_declared_output(oracle, name):
    c = oc.CASES[name]
    o_np, o_orc = outputs(numpy_ref, name), outputs(oracle, name)
    oc.check_declared(c, o_np)
    oc.check_declared(c, o_orc)
    pk, xk = ("poses", "points") if c.call == "ba" else ("pose", "points")
    for a, b in zip(np.atleast_2d(o_np[pk]), np.atleast_2d(o_orc[pk])):  # the two implementations against each other
        assert max(pose_err(a, b)) < 1e-8, (name, pose_err(a, b))
    if xk in o_np:
        np.testing.assert_allclose(o_np[xk], o_orc[xk], rtol=0, atol=1e-7, err_msg=name)
    for k in c.want.get("frozen_points", ()):  # (the oracle has no instrumentation: its frozen vertex is numpy_ref's, whose bits are those of round 2)
        np.testing.assert_allclose(o_orc["points"][k], o_np["points"][k], rtol=0, atol=1e-9)
    for k in c.want.get("frozen_poses", ()):
        assert max(pose_err(o_orc["poses"][k], o_np["poses"][k])) < 1e-9
    if c.call == "anchored":
        assert np.array_equal(o_np["d2"] <= 9.0, o_orc["d2"] <= 9.0) and np.allclose(o_np["d2"], o_orc["d2"], rtol=1e-9, atol=0), name
        rel = oc.related_data(c)
        if rel is not None:  # the twin without the column or slot, or the case this one moves further than: on the same implementation
            oc.check_related(c, o_np, oc.run(numpy_ref, "anchored", rel))
            oc.check_related(c, o_orc, oc.run(oracle, "anchored", rel))


@pytest.mark.parametrize("name", sorted(oc.CONVERTED))
def test_converted_case_is_the_case_it_came_from(oracle, name):
    """anchored_from_ba re-expresses a local-BA case in the dense layout of gl_track_frames_anchored: the oracle on the case as written ("ba")
    and on the converted one ("anchored") gives the same erase mask, the same dropped associations and the same pose to 1e-12."""
    c = oc.CASES[name]
    ba_name, slot = oc.CONVERTED[name]
    b = oc.CASES[ba_name]
    o_ba, o_an = outputs(oracle, ba_name), outputs(oracle, name)
    erase = np.array([o_an["own_erase"][l] if j < 0 else o_an["fixed_erase"][l, j] for l, j in slot], np.uint8)
    assert np.array_equal(erase, o_ba["erase"]) and np.array_equal(o_an["assoc"], np.where(o_ba["dropped"] == 1, -1, b.data["assoc"])), name
    assert max(pose_err(o_an["pose"], o_ba["poses"][0])) < 1e-12 and np.abs(o_an["points"] - o_ba["points"]).max() < 1e-12, name


BANDED = [n for n in NAMES if oc.CASES[n].band]


@pytest.mark.parametrize("name", BANDED)
def test_banded_case_sits_in_its_band(oracle, name):
    b = oc.CASES[name].band
    inside = oc.in_float_gap if b["side"] == "float" else (lambda q: oc.in_band(q, b["thr"], b["side"]))
    q_np, q_orc = b["q"](numpy_ref), b["q"](oracle)
    assert inside(q_np), (name, q_np / b["thr"] - 1)
    if q_orc is not None:  # (a chi2 a verdict was taken on half-way is no output: the oracle is then held by its decision on either side)
        assert inside(q_orc), (name, q_orc / b["thr"] - 1)


def test_banded_cases_come_in_both_sides():
    for n in BANDED:
        if oc.CASES[n].band["side"] == "float":
            continue
        other = n.replace("_below", "_above") if n.endswith("_below") else n.replace("_above", "_below")
        assert other in oc.CASES and oc.CASES[other].band["side"] != oc.CASES[n].band["side"], n


def test_stale_chi2_would_pass_when_recomputed():
    """ba.stale_erase: the recomputed chi2 of the erased observation is below the threshold, the one it was erased on above"""
    tr = outputs(numpy_ref, "ba_stale_erase")["trace"]
    assert tr["obs_fresh"][1] < 0.9 * oc.TH_MONO and tr["obs_erase"][1] > 1.1 * oc.TH_MONO and tr["obs_erase"][1] == tr["obs_level"][1]


def test_every_decision_has_two_sides_and_an_alteration():
    sides = {}
    for c in oc.CASES.values():
        sides.setdefault(c.decision, set()).add(c.side)
    assert set(sides) == set(oc.DECISIONS)
    for d in oc.DECISIONS:
        assert len(sides[d]) >= 2, (d, sides[d])
    assert set(ALTERED) == set(oc.DECISIONS)


# ---- stability ------------------------------------------------------------------------------------------------------------------------
INTS = {"pose": ("outl", "nin"), "ba": ("dropped", "erase"), "track": ("assoc",), "anchored": ("assoc", "fixed_erase")}


def reorder(c, rng):
    """the case with its edges in another order -> (data, back): back(o) brings the outputs to the case's order.  (_reorder_spread of
    tests/test_gpu_soak_cases.py returns the spread of ONE pose over a permutation of n points; here the integers of every re-ordered run
    are compared too, and a local-BA case also re-orders the observations within each point.)"""
    d = dict(c.data)
    if c.call in ("pose", "track"):
        perm = rng.permutation(len(d["oct"]))
        for k in ("Xw", "obs", "oct"):
            d[k] = c.data[k][perm]

        def back(o):
            o = dict(o)
            for k in ("outl", "assoc", "points", "d2"):
                if k in o:
                    v = np.empty_like(o[k])
                    v[perm] = o[k]
                    o[k] = v
            return o
        return d, back
    if c.call == "anchored":  # the point slots and the fixed columns
        perm, cperm = rng.permutation(len(d["oct"])), rng.permutation(len(d["fixed_pose"]))
        for k in ("Xw", "obs", "oct"):
            d[k] = c.data[k][perm]
        d["fixed_pose"] = c.data["fixed_pose"][cperm]
        d["fixed_obs"], d["fixed_oct"] = c.data["fixed_obs"][np.ix_(perm, cperm)], c.data["fixed_oct"][np.ix_(perm, cperm)]

        def back(o):
            o = dict(o)
            for k in ("assoc", "points", "d2", "own_erase"):
                v = np.empty_like(o[k])
                v[perm] = o[k]
                o[k] = v
            v = np.empty_like(o["fixed_erase"])
            v[np.ix_(perm, cperm)] = o["fixed_erase"]
            o["fixed_erase"] = v
            return o
        return d, back
    L = len(d["points"])
    perm = rng.permutation(L)  # the points, and the observations within each point
    sel = np.concatenate([rng.permutation(np.arange(d["obs_ptr"][l], d["obs_ptr"][l + 1])) for l in perm]).astype(int)
    d["obs_ptr"] = np.concatenate([[0], np.cumsum(np.diff(c.data["obs_ptr"])[perm])]).astype(np.int32)
    for k in ("obs_pose", "obs_uvr", "obs_oct"):
        d[k] = c.data[k][sel]
    d["points"], d["assoc"] = c.data["points"][perm], c.data["assoc"][perm]

    def back(o):
        o = dict(o)
        for k, p in (("points", perm), ("dropped", perm), ("erase", sel)):
            v = np.empty_like(o[k])
            v[p] = o[k]
            o[k] = v
        return o
    return d, back


FLOAT_KEYS = {"pose": ("pose", "Xw", "obs"), "track": ("pose", "Xw", "obs", "mean", "cov"), "ba": ("poses", "points", "obs_uvr", "mean", "cov"),
              "anchored": ("pose", "Xw", "obs", "fixed_pose", "fixed_obs", "mean", "cov")}


def one_ulp(c, rng):
    """the case with ONE input moved by one ulp (ulp_variants of tests/test_gpu_soak_cases.py), drawn again while it hits what the case
    exempts: the solved scalar, the bits a decision is about, a monocular marker"""
    fixed = {(k, i) for k, i in c.fixed}
    while True:
        k = FLOAT_KEYS[c.call][int(rng.integers(len(FLOAT_KEYS[c.call])))]
        a0 = np.array(c.data[k], float)
        a = ulp_variants(a0, 1, rng)[0]
        i = tuple(int(x) for x in np.argwhere(a != a0)[0])
        if (k, None) in fixed or (k, i) in fixed or (k in ("obs", "obs_uvr", "fixed_obs") and i[-1] == 2 and a0[i] < 0):
            continue
        return dict(c.data, **{k: a})


@pytest.mark.parametrize("name", NAMES)
def test_case_is_stable(oracle, name):
    """The condition of entry: the declared integers do not depend on the order of the edges or on an ulp of an input, and the oracle's pose
    moves by less than the parity tolerance.  An exact scene (iters == 1, outputs unchanged by the bytes) stays exact under re-ordering
    only - one ulp on an input makes its residual non-zero - so its `iters` and `unchanged` are held in the re-ordered runs alone."""
    c = oc.CASES[name]
    ref = outputs(oracle, name)
    rng = np.random.default_rng(len(name))
    pk = "poses" if c.call == "ba" else "pose"
    for probe in range(48):  # (an "anchored" case: the 12 re-orderings permute its point slots and its fixed columns)
        if probe < 12:
            d, back = reorder(c, rng)
            o = back(oc.run(oracle, c.call, d))
            want = c.want
        else:
            d = one_ulp(c, rng)
            o = oc.run(oracle, c.call, d)
            want = {k: v for k, v in c.want.items() if k not in ("iters", "unchanged", "unchanged_poses", "pose_bytes", "d2_of", "outer")}
        for k in INTS[c.call]:
            assert np.array_equal(o[k], ref[k]), (name, probe, k)
        oc.check_declared(c, o, want=want, data=d if c.call == "anchored" and probe >= 12 else None)
        for a, b in zip(np.atleast_2d(o[pk]), np.atleast_2d(ref[pk])):
            assert max(pose_err(a, b)) < 1e-6, (name, probe, pose_err(a, b))


# ---- that the tests bite ---------------------------------------------------------------------------------------------------------------
UP, DOWN = 1 + 1e-5, 1 - 1e-5
ALTERED = {
    "pose.chi2_mono": [dict(chi2_mono=5.991 * UP), dict(chi2_mono=5.991 * DOWN)],
    "pose.chi2_stereo": [dict(chi2_stereo=7.815 * UP), dict(chi2_stereo=7.815 * DOWN)],
    "pose.float_cast": [dict(cast=float)],
    "pose.mono_by_uright": [dict(is_mono=lambda ur: ur <= 0), dict(is_mono=lambda ur: bool(np.signbit(ur))), dict(is_mono=lambda ur: ur < -1e-300)],
    "pose.readmit": [dict(readmit=False)],
    "pose.all_outliers_later": [dict(min_active=3)],
    "ba.obs_chi2_mono": [dict(chi2_mono=5.991 * UP), dict(chi2_mono=5.991 * DOWN)],
    "ba.obs_chi2_stereo": [dict(chi2_stereo=7.815 * UP), dict(chi2_stereo=7.815 * DOWN)],
    "ba.float_vs_double": [dict(cast=F32)],
    "ba.depth": [dict(depth_test=False)],
    "ba.stale_erase": [dict(stale=False)],
    "ba.str_level": [dict(str_level_scale=UP), dict(str_level_scale=DOWN)],
    "ba.str_drop": [dict(str_drop_scale=UP), dict(str_drop_scale=DOWN)],
    "ba.nondegenerate": [dict(str_all=True)],
    "ba.assoc_none": [dict(gate=lambda d2: d2 < 9.0), dict(gate=lambda d2: d2 <= 9.0 + 4e-15), dict(assoc_of=lambda a: np.maximum(a, 0))],
    "ba.vertex_leaves": [dict(ignore_level_last=True)],
    # (keep_all alone - the empty block of the unobserved key-frame kept in the system - changes nothing: lambda damps it and its step is 0.
    # That is what the device does.  What makes it wrong is the block kept WITHOUT its damping: the system is singular and nothing moves)
    "ba.pose_unobserved": [dict(keep_all=True, lam_scale=0.0)],
    "ba.single_mono": [dict(lam_scale=0.0)],
    "ba.prior_or_fixed": [dict(prior_as_edge=True), dict(prior_as_edge=False)],
    "lm.rho_zero": [dict(rho_stop=False)],
    "lm.reject": [dict(raise_lambda=False)],
    "fx.chi2_level": [dict(chi2_mono=5.991 * UP, chi2_stereo=7.815 * UP), dict(chi2_mono=5.991 * DOWN, chi2_stereo=7.815 * DOWN)],
    "fx.depth": [dict(depth_test=False), dict(depth_pose=lambda j: 0)],  # (no depth test; the depth taken in the frame's camera)
    "fx.depth_own_camera": [dict(depth_pose=lambda j: 0)],
    "fx.stale_erase": [dict(stale=False)],
    "fx.mono_by_uright": [dict(is_mono=lambda ur: ur <= 0), dict(is_mono=lambda ur: bool(np.signbit(ur))), dict(is_mono=lambda ur: ur < -1e-300)],
    "fx.not_observed": [dict(observed=lambda fo: fo >= -1)],
    "fx.point_keeps_fixed_edges": [dict(ignore_level_last=True)],
    "fx.point_leaves": [dict(ignore_level_last=True)],
    "fx.str_level": [dict(str_level_scale=UP), dict(str_level_scale=DOWN)],
    "fx.str_drop": [dict(str_drop_scale=UP), dict(str_drop_scale=DOWN)],
    "fx.prior_or_fixed": [dict(prior_as_edge=True), dict(prior_as_edge=False)],
    "fx.float_vs_double": [dict(cast=F32)],
}
ALTERATIONS = [(d, i) for d in sorted(ALTERED) for i in range(len(ALTERED[d]))]


@pytest.mark.parametrize("decision,i", ALTERATIONS, ids=["%s-%d" % a for a in ALTERATIONS])
def test_altered_comparison_changes_a_declared_output(decision, i):
    """numpy_ref with ONE comparison altered - a threshold moved by a relative 1e-5, the float cast removed or added, `<` for `<=`, the
    depth test removed, the stale chi2 recomputed ... -: at least one case of the decision no longer gives what it declares."""
    alt = ALTERED[decision][i]
    missed = []
    for n in NAMES:
        c = oc.CASES[n]
        if c.decision != decision:
            continue
        if misses(c, alt):
            missed.append(n)
    assert missed, (decision, sorted(alt))


_missed = {}


def misses(c, alt):
    """whether numpy_ref with the alteration no longer gives what the case declares; None where the alteration does not apply to the call"""
    if (c.name, id(alt)) not in _missed:  # (alt: one of ALTERED's dicts; the three tests below ask about the same pairs)
        _missed[c.name, id(alt)] = _misses(c, alt)
    return _missed[c.name, id(alt)]


def _misses(c, alt):
    if ("gate" in alt) != (c.call in ("track", "anchored")) and ("gate" in alt or "assoc_of" in alt):
        return None  # (the gate is gl_track_frames' and the anchored call's, the meaning of assoc < 0 the local BA's)
    try:
        with np.errstate(all="ignore"):  # (an undamped singular system overflows: that is the point of that alteration)
            o = oc.run(numpy_ref, c.call, c.data, trace=True, **alt)
        if c.call in ("track", "anchored"):
            o["outer"] = sum(len(t["q"]) for t in o["trace"]["lm"])
        oc.check_declared(c, o)
    except (AssertionError, np.linalg.LinAlgError):
        return True
    return False


ANCHORED_ALTERATIONS = [(d, i) for d, i in ALTERATIONS if any(c.decision == d for c in oc.CASES.values() if c.call == "anchored") and "assoc_of" not in ALTERED[d][i]]


@pytest.mark.parametrize("decision,i", ANCHORED_ALTERATIONS, ids=["%s-%d" % a for a in ANCHORED_ALTERATIONS])
def test_altered_comparison_changes_an_anchored_output(decision, i):
    """The same on the cases of gl_track_frames_anchored alone: every decision that has "anchored" cases is held by one of THEM."""
    assert [n for n in oc.names("anchored") if oc.CASES[n].decision == decision and misses(oc.CASES[n], ALTERED[decision][i])], (decision, i)


@pytest.mark.parametrize("name", [n for n in BANDED if oc.CASES[n].call == "anchored" and oc.CASES[n].band["side"] != "float"])
def test_anchored_threshold_case_bites(name):
    """every "anchored" case at a threshold, on its own: the threshold moved by a relative 1e-5 to its side changes a declared output"""
    c = oc.CASES[name]
    assert any(misses(c, alt) for alt in ALTERED[c.decision]), name
