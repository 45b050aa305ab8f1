"""CPU: GL_ASSOC_SCREENED's fp32 bound held to exact arithmetic, and its declared cases (tests/assoc_screen_cases.py) held to the
bit-exact model of tests/assoc_screen_model.py.  The device is held to the same declarations in tests/test_gpu_assoc_screen_cases.py.

  * THE BOUND: float(lo) <= chi2_device(record, p) <= float(hi) for every pair of six families (3 000 and more pairs each, pinned
    seeds) - the inequality the kernel's answer rests on - and, where the pair is well scaled, the same against chi2_exact in rational
    arithmetic, widened by item (4) of the proof (the fp64 evaluation's own error, taken as 1e-14 c ||d||^2);
  * teeth: without the beta term the far-origin family violates it; with the verify kernel's re-test turned strict the declared
    counts of every ladder change; with a compaction that drops the entries equal to U the declared fallback of compact.cap4 changes;
  * every declared case: the launch shape it was built to reach, the path through note() it was built to take, idx / d2 equal to
    chi2_device's first minimum, (idx, verified, fallback) equal to the declaration, every fp32 intermediate zero or normal.

The worst |s - chi2| / e per family, measured with this file (tightness_table() prints it again; DESIGN.md has it next to the bound):
    iso 0.215   aniso 0.125   offdiag 0.142   far 0.200   near 0.133   gate 8.0e-11
"""
import math

import numpy as np
import pytest

from tests import assoc_screen_cases as sc
from tests import assoc_screen_model as sm

Fr = sm.Fr
f32 = np.float32


# ---- the model's own pieces ---------------------------------------------------------------------------------------------------------------
def test_round_f32_rounds_once_to_nearest_even():
    rng = np.random.default_rng(1)
    for _ in range(5000):  # a double rounds to fp32 once either way
        x = float(rng.standard_normal() * 10.0 ** rng.uniform(-44, 38))
        assert sm.round_f32(Fr(x)).tobytes() == f32(x).tobytes(), x
    one, ulp = Fr(1), Fr(1, 2 ** 23)
    assert sm.round_f32(one + ulp / 2) == f32(1.0)                      # a tie: to even, down
    assert sm.round_f32(one + 3 * ulp / 2) == f32(1.0 + 2.0 ** -22)     # a tie: to even, up
    x = one + ulp / 2 + Fr(1, 2 ** 60)                                  # just above a tie: up; through a double it would go down
    assert sm.round_f32(x) == f32(1.0 + 2.0 ** -23) and f32(float(x)) == f32(1.0)
    assert sm.round_f32(Fr(2) ** 128 - Fr(2) ** 103) == f32(np.inf) and sm.round_f32(Fr(2) ** 128 - Fr(2) ** 103 - 1) == np.finfo(f32).max
    assert sm.round_f32(Fr(1, 2 ** 150)) == 0.0 and sm.round_f32(Fr(3, 2 ** 150)) == f32(2.0 ** -148)  # subnormals: 0.5 and 1.5 last places, ties to even
    assert sm.fmaf(f32(3.0), f32(1.0 + 2.0 ** -23), f32(-3.0)) == f32(3.0 * 2.0 ** -23)  # exact where the product alone would round


def test_constants_are_the_sources():
    c = sm.source_constants()
    assert c["kCap"] % 2 == 0 and c["kOut"] <= c["kCap"] // 2  # both instantiations can fill kOut
    assert (c["kCap"], c["kOut"], c["kLimit"], c["G0"], c["G1"], c["F1"], c["F2"], c["beta_u"], c["beta_floor"], c["big"]) == \
        (8, 4, 1e37, 2.0 ** -20, 2.5, 2.5, 8.0, 1.01, 1e-30, 3.1)  # the figures the pinned cases were searched under


def test_model_gives_the_sweeps_answer_on_a_random_map():
    from gmmloc_amd import synth
    mean, cov = synth.synth_gmm(96, 4)
    m = sm.ScreenMap(mean, cov)
    for p in synth.synth_points(mean, cov, 12, 5):
        r = sm.associate_point(m, p, 12)
        assert (r.idx, r.d2) == sm.exhaustive(m, p) and not r.fell_back and r.verified >= 1


def test_restated_shapes():
    """the shapes the issue's cases rest on, by the restated screen_shape / sweep_split / sweep_points"""
    S = sm.screen_shape
    assert [S(K, 2)["nsplit"] for K in (65, 72, 128, 129)] == [2, 2, 2, 3]
    assert S(2304, 8191) == dict(ppt=2, ptiles=16, nsplit=32, kchunk=72, chunks=9, cap=8, L=8)
    assert S(2304, 8192)["ppt"] == 2 and S(80, 16383)["ppt"] == 2 and S(80, 16384) == dict(ppt=4, ptiles=16, nsplit=2, kchunk=40, chunks=5, cap=4, L=1)
    assert [(S(K, 4)["nsplit"], S(K, 4)["L"]) for K in (256, 257, 1024, 1025, 2049)] == [(4, 1), (5, 2), (16, 4), (17, 8), (33, 16)]
    assert sm.sweep_points(100, True) == 256 and sm.sweep_points(16 * 300, True) == 300 and S(4096, 16 * 16384, True)["ppt"] == 4


# ---- THE BOUND -------------------------------------------------------------------------------------------------------------------------------
def bound_check(name, **mutation):
    """(pairs, violations, worst |s - chi2| / e) over the family; the exact check on the well-scaled families"""
    pairs, bad, worst = 0, [], 0.0
    for mean, cov, pts in sc.family(name):
        m = sm.ScreenMap(mean, cov)
        assert m.r32 is not None
        for p in pts:
            q = sm.screen_point(m, p, **mutation)
            assert q.ok, (name, p, q.big)
            for k in range(m.K):
                tr = {}
                hi, lo = sm.pair(m.r32[k], q, strict=False, trace=tr)
                chi2 = sm.chi2_device(m.rec[k], p)
                pairs += 1
                e = float(tr["E"]) * float(q.G)
                if e > 0 and math.isfinite(e):
                    worst = max(worst, abs(float(tr["s"]) - chi2) / e)
                if not (float(lo) <= chi2 <= float(hi)) or not (math.isfinite(float(lo)) and math.isfinite(float(hi))):
                    bad.append((k, tuple(p), float(lo), chi2, float(hi)))  # (a screened point's fp32 values stay finite: the `ok` gate)
                elif name in sc.WELL_SCALED and not mutation:
                    d = p - mean[k]
                    w = Fr(1e-14 * float(m.r32[k][9]) * float(d @ d))
                    ex = sm.chi2_exact(cov[k], mean[k], p)
                    if not (Fr(float(lo)) - w <= ex <= Fr(float(hi)) + w):
                        bad.append(("exact", k, tuple(p), float(lo), float(ex), float(hi)))
    return pairs, bad, worst


def tightness_table():
    for name in sc.FAMILY_SEED:
        print(name, "%d pairs, worst |s - chi2| / e = %.3f" % bound_check(name)[::2])


@pytest.mark.parametrize("name", list(sc.FAMILY_SEED))
def test_bound_holds_on_family(name):
    pairs, bad, worst = bound_check(name)
    print(name, pairs, worst)
    assert pairs >= 3000
    assert not bad, (len(bad), bad[:3])
    assert worst <= 1.0


def test_bound_needs_its_beta_term():
    """teeth: with beta = 0 (G = 2^-20, F = 0) the rounding of coordinates 1e3 .. 1e6 m from the origin is not paid for"""
    pairs, bad, worst = bound_check("far", beta_zero=True)
    print(len(bad), "of", pairs, "pairs violate, worst", worst)
    assert len(bad) > pairs // 10 and worst > 1.0


# ---- the declared cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_declared_case(name):
    c = sc.CASES[name]
    got = sm.screen_shape(c.K, c.N)
    assert {k: got[k] for k in c.shape} == c.shape, got              # the shape the case was built to reach
    assert (c.map().r32 is not None) == c.has_records
    res, ref = c.model(), c.reference()                              # strict: a subnormal or infinite fp32 intermediate raises
    for i, r in enumerate(res):
        assert (r.idx, r.d2) == (int(ref["idx"][i]), float(ref["d2"][i])), (name, i, r[:4])   # chi2_device's first minimum
        assert (r.idx, r.verified, int(r.fell_back)) == tuple(sc.DECLARED[name][i]), (name, i, r[:4])
        if sc.HAND.get(name) and sc.HAND[name][i] is not None:
            assert r.idx == sc.HAND[name][i], (name, i, r.idx)
    for i, want in c.reach.items():                                  # the path through note()
        s = res[i].splits[want["split"]]
        assert (s.compactions, s.peak) == (want["compactions"], want["peak"]), (name, i, s)
    assert c.counters() == (sum(m * r.verified for m, r in zip(c.multiplicity(), res)), sum(m * int(r.fell_back) for m, r in zip(c.multiplicity(), res)))


def _step(m, p, k0, k1, N):
    q = sm.screen_point(m, p)
    return sm.pair(m.r32[k0], q)[0], sm.pair(m.r32[k1], q)[1], sm.associate_point(m, p, N)


def _assert_step(m, eq, up, k0, k1, N):
    """lo_k1 == U = hi_k0 exactly at `eq`, one fp32 ulp above at `up`; the two are adjacent doubles of x"""
    assert eq[1:] == up[1:] and abs(eq[0] - up[0]) == math.ulp(min(eq[0], up[0]))
    h, l, r = _step(m, eq, k0, k1, N)
    assert r.U == h and l == h
    h, l, r = _step(m, up, k0, k1, N)
    assert r.U == h and l == np.nextafter(h, f32(np.inf))


def _sensitive(m, pts, N, ks, group):
    """does moving one intermediate of `group`, of one of the components ks, by one ulp change (verified, fallback) of a point?"""
    for p in pts:
        base = sm.associate_point(m, p, N)
        for stage in sc.GROUPS[group]:
            for k in ks:
                for u in (1, -1):
                    r = sm.associate_point(m, p, N, nudge=(k, {stage: u}))
                    if (r.verified, r.fell_back) != (base.verified, base.fell_back):
                        return True
    return False


@pytest.mark.parametrize("K", sorted(sc.LADDERS))
def test_ladder_edge(K):
    """two adjacent doubles; `verified` steps from 2 to 1; a one-ulp change of each listed intermediate changes the count"""
    c_eq, c_up = sc.CASES["ladder.K%d.n1.eq" % K], sc.CASES["ladder.K%d.n1.up" % K]
    eq, up = tuple(c_eq.pts[0]), tuple(c_up.pts[0])
    _assert_step(c_eq.map(), eq, up, 0, 1, 1)
    assert [d[1] for d in (sc.DECLARED[c_eq.name][0], sc.DECLARED[c_up.name][0])] == [2, 1]
    for group in sc.DECIDES[K]:
        assert _sensitive(c_eq.map(), (eq, up), 1, (0, 1), group), group


def test_ladder_near_a_mean_and_the_deciding_roundings():
    c = sc.CASES["ladder.near.eq"]
    eq, up = tuple(c.pts[0]), tuple(c.pts[1])
    _assert_step(c.map(), eq, up, 0, 1, 2)
    assert [d[1] for d in sc.DECLARED[c.name]] == [2, 1]
    for group in sc.DECIDES["near"]:
        assert _sensitive(c.map(), (eq, up), 2, (0, 1), group), group
    # every group of intermediates decides some ladder: D, t0 / t1 / t2, s, n / E, the final fma of hi / lo
    assert set(sc.GROUPS) == set(g for v in sc.DECIDES.values() for g in v)


def test_mutation_strict_retest_changes_every_ladder():
    """teeth: a verify kernel that skips a component at lo >= U loses the one with lo == U (one evaluation less per ladder call with
    such a point); the calls whose point is one ulp above are as declared"""
    for n in sc.names("ladder."):
        c = sc.CASES[n]
        mut = c.counters([(r.idx, r.verified, int(r.fell_back)) for r in c.model(retest_strict=True)])
        ver, fb = c.counters()
        assert mut == ((ver - 1, fb) if ".eq" in n or ".near." in n else (ver, fb)), (n, mut, ver, fb)


def test_mutation_compaction_dropping_equal_entries_changes_the_tie():
    c = sc.CASES["compact.cap4"]
    eq, up = tuple(c.pts[5]), tuple(c.pts[6])
    _assert_step(c.map(), eq, up, 5, 13, c.N)
    assert [tuple(d) for d in sc.DECLARED[c.name][5:7]] == [(5, 0, 1), (5, 4, 0)]  # lo == U: kept, so no room: fallback; above: never noted
    mut = [(r.idx, r.verified, int(r.fell_back)) for r in c.model(compact_drops_equal=True)]
    assert mut[5] == (5, 4, 0) and mut[:5] + mut[6:] == [tuple(d) for d in sc.DECLARED[c.name][:5] + sc.DECLARED[c.name][6:]]
    assert c.counters(mut) != c.counters()
    for group in sc.DECIDES["tie"]:
        assert _sensitive(c.map(), (eq, up), c.N, (5, 13), group), group


def test_gates_sit_between_adjacent_doubles():
    c = sc.CASES["gate.point"]
    lim = float(f32(sm.source_constants()["kLimit"]))
    q0, q1 = sm.screen_point(c.map(), c.pts[0]), sm.screen_point(c.map(), c.pts[1])
    assert q0.ok and q0.big <= lim < q1.big and not q1.ok
    assert [d[2] for d in sc.DECLARED[c.name]] == [0, 1, 0]
    a, b = sc.CASES["gate.map.below"].map(), sc.CASES["gate.map.above"].map()
    assert a.r32 is not None and a.cmax * (a.rmax * a.rmax) < 1e30 <= b.cmax * (b.rmax * b.rmax) and b.r32 is None
    assert [d[2] for d in sc.DECLARED["gate.map.above"]] == [1, 1, 1]
    bad = sm.ScreenMap(np.array([[0.0, 0, 0], [1.0, 0, 0]]), np.array([np.eye(3) * 1e-41, np.eye(3)]))  # cov_inv 1e41: not an fp32 number
    assert bad.r32 is None
