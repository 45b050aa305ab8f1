"""The hand-built key-frame cases (tests/keyframe_cases.py) on the CPU: the C++ oracle and oracle/numpy_ref.py both give the output every
case declares, the banded cases sit where they say on both, the pairs differ in one element, every decision has two sides, the ties
are bit-equal and the regime scenes enter their regime.

That the cases can fail: one constant or comparison of a scratch copy of the oracle changed at a time, and the cases that then miss their
declared output (the first three, and their number).  view.cap, corr.nfeat, pt.skip and tri.skip are what include/gmmloc_hip.h states for inputs
the reference never sees; keyframe_cases.run() applies them for both CPU implementations, so their mutants change run().
  view.cos            78 -> 78.001 deg                                           view_cos_below
  view.cos            the cos test applied to every component                    view_cos_nondegenerate_at_the_angle, view_cov2d_both_exactly_4, view_cov2d_one_above
  view.behind         z > 0 -> z > -2                                            corr_view_of_0_k5, view_z_negative_projects_inside
  view.image          u < width -> <=                                            view_cx_width_on_axis, view_u_width
  view.image          v < height -> <=                                           view_v_height
  view.image          u >= 0 -> > 0                                              view_cx_0_on_axis, view_u_0
  view.image          v >= 0 -> > 0                                              view_v_0
  view.cov2d          4.0 -> 4.00001                                             view_cov2d_both_exactly_4, view_cov2d_one_above
  view.cov2d          < -> <= (both)                                             view_cov2d_both_exactly_4
  view.merge          0.8 -> 0.79                                                view_merge_bh_below
  view.merge          depth < -> <=                                              view_merge_equal_depth_old_stays
  view.merge          argmin: last of equals                                     view_merge_equal_distance_first_slot
  view.merge          farther replaces too                                       view_merge_equal_depth_old_stays, view_merge_farther_discarded, view_order_met_and_discarded_across_rounds ... (5)
  view.merge_order    distances to the list as a round of 16 found it            view_order_chain_one_round, view_order_same_argmin_across_rounds, view_order_met_and_discarded_old_slot ... (12)
  view.sort           equal depths by id                                         view_sort_equal_depth_list_order
  view.sort           ascending                                                  corr_nfeat_0, corr_nfeat_1, corr_nfeat_all ... (27)
  view.cap            nview counts what view_ids holds                           view_cap_above
  view.cap            view_ids holds the last view_cap                           view_cap_above
  corr.gate           9.0 -> 8.99                                                corr_gate_below
  corr.gate           gate off                                                   corr_euclidean_order_k1, corr_euclidean_order_k2, corr_gate_above ... (6)
  corr.knn_then_gate  the k nearest that pass (k + 1 searched)                   corr_euclidean_order_k1, corr_knn_then_gate_k2
  corr.fewer_than_k   unused slots padded with 0                                 chain_view_of_two_planes, corr_euclidean_order_k1, corr_euclidean_order_k2 ... (13)
  corr.fewer_than_k   ncand = the number searched                                chain_view_of_two_planes, corr_euclidean_order_k1, corr_euclidean_order_k2 ... (13)
  corr.tie            knn: later of equals first                                 cma_fallback_tie_K16_up0_down15, cma_fallback_tie_K16_up15_down0, cma_fallback_tie_K17_up0_down16 ... (11)
  corr.nfeat          nfeat ignored                                              corr_nfeat_0, corr_nfeat_1
  pt.chi2_proj        7.815 -> 7.8                                               pt_chi2_proj_below
  pt.chi2_str         threshold * 1.00001                                        pt_chi2_str_above
  pt.chi2_str         check always on                                            pt_chi2_str_above_check_off
  pt.solver_fail      an update applied after a failed solve                     pt_solver_fail
  pt.solver_fail      a failed solve does not stop the iterations                none: without an update every later iteration repeats the first
  pt.skip             octave 8 solved                                            pt_skip_octave_8
  pt.skip             comp K solved                                              pt_skip_comp_K
  pt.skip             a skipped problem reports res 1                            pt_skip_comp_K, pt_skip_comp_minus_1, pt_skip_octave_8 ... (4)
  cma.empty           empty list goes on                                         cma_ncand_0
  cma.first_min       < -> <=                                                    cma_duplicate_higher_index_first, cma_duplicate_lower_index_first
  cma.neighbour       ln < ll -> <=                                              cma_duplicate_higher_index_first, cma_duplicate_lower_index_first, cma_neighbour_bit_equal ... (4)
  cma.neighbour       no neighbour scan                                          cma_20_neighbours_winner_at_0, cma_20_neighbours_winner_at_15, cma_20_neighbours_winner_at_16 ... (6)
  cma.neighbour       failed switch keeps the neighbour's ll                     cma_switch_fails_own_chi2_rejects
  cma.neighbour       failed switch keeps the neighbour                          cma_switch_fails_back_to_candidate
  cma.gate            9.0 -> 8.99                                                cma_gate_below
  cma.fallback        non-degenerate tried too                                   cma_fallback_not_degenerate
  cma.fallback        fallback result ignored                                    cma_all_minus_1, cma_fallback_degenerate_moves, cma_fallback_tie_K16_up0_down15 ... (8)
  cma.fallback        failed fallback moves                                      cma_fallback_K1, cma_fallback_fails
  cma.proj_z          no clamp                                                   cma_20_neighbours_winner_at_0, cma_20_neighbours_winner_at_15, cma_20_neighbours_winner_at_16 ... (9)
  cma.proj_z          no scaling                                                 cma_proj_z_half
  tri.dedup           dedup keeps the last occurrence                            tri_first_occurrence_counts_across_lists, tri_first_occurrence_counts_in_cand1
  tri.dedup           dedup off  none: a repeated candidate repeats its sum bit for bit (equivalent)
  tri.degenerate_only all candidates                                             tri_best_not_degenerate, tri_none_degenerate
  tri.first_min       < -> <=                                                    tri_duplicate_across_lists_higher_first, tri_duplicate_across_lists_lower_first
  tri.chi2            7.8 -> 7.79 (kf1)                                          tri_e1_stereo_below
  tri.chi2            7.8 -> 7.79 (kf2)                                          tri_e2_stereo_below
  tri.chi2            5.991 -> 5.99                                              tri_e1_mono_below, tri_e2_mono_below, tri_oct2_ignored
  tri.chi2            kf2 weighed with oct2                                      tri_oct2_ignored_above
  tri.chi2            u_right -0.0 is mono                                       tri_u_right_minus_0
  tri.chi2_str        threshold * 1.00001                                        tri_chi2_str_above
  tri.chi2_str        check always on                                            tri_chi2_str_above_check_off
  tri.skip            octave 8 solved                                            tri_skip_oct1_8
  tri.skip            a skipped match reports component 0                        tri_skip_oct1_8, tri_skip_oct1_minus_1
  cmp.parallax        0.9998 -> 0.99981                                          cmp_mono_parallax_at_0.9998
  cmp.parallax        > 0 -> >= 0                                                cmp_rays_90_degrees, cmp_rays_90_degrees_stereo1
  cmp.parallax        depth2 read with both stereo                               cmp_stereo_both_depth2_unread
  cmp.parallax        no stereo branch 2                                         cmp_project_u1_0, cmp_project_u1_width, cmp_stereo2_narrow
  cmp.parallax        cosStereo test off                                         cmp_project_u1_0, cmp_project_u2_0, cmp_reproj_kf1_oct0_below ... (19)
  cmp.depth_vs_uright stereo by depth                                            cmp_u_right_without_depth
  cmp.depth_vs_uright b1 / b2 keep u_right without a depth                       cmp_u_right_without_depth_mono_edge
  cmp.project         u < width -> <=                                            cmp_project_u1_width, cmp_project_u2_width
  cmp.project         u >= 0 -> > 0                                              cmp_project_u1_0, cmp_project_u2_0
  cmp.project         behind test off                                            cmp_project_behind_1, cmp_project_behind_2
  cmp.reproj          7.8 -> 7.79 (kf1)                                          cmp_reproj_kf1_oct0_below, cmp_reproj_kf1_oct3_below
  cmp.reproj          5.991 -> 5.99 (kf2)                                        cmp_reproj_kf2_oct0_below, cmp_reproj_kf2_oct3_below
  cmp.reproj          kf2 with oct2's sigma                                      cmp_reproj_kf2_oct0_above, cmp_reproj_kf2_oct3_below
  cmp.reproj          5.991 -> 5.99 (kf1)                                        cmp_reproj_kf1_mono_oct0_below, cmp_reproj_kf1_mono_oct3_below
  cmp.reproj          7.8 -> 7.79 (kf2)                                          cmp_reproj_kf2_stereo_oct0_below, cmp_reproj_kf2_stereo_oct3_below
  cmp.scale           > -> >= (upper)                                            cmp_scale_upper_at_1.2, cmp_scale_upper_at_1.25, cmp_scale_upper_octaves_at_1.25
  cmp.scale           < -> <= (lower)                                            cmp_scale_lower_at_1.2, cmp_scale_lower_at_1.25
  cmp.scale           factor 1.5 -> 1.5000001                                    cmp_scale_lower_below_1.2, cmp_scale_lower_below_1.25, cmp_scale_upper_above_1.2 ... (5)
  cmp.type            GMM types swapped                                          cmp_mono_parallax_below_0.9998, cmp_project_u1_0, cmp_project_u2_0 ... (22)
  cmp.type            mono / stereo swapped                                      cmp_mono_parallax_below_0.9998, cmp_project_u1_0, cmp_project_u2_0 ... (22)
"""
import warnings

import numpy as np
import pytest

from oracle import numpy_ref
from tests import keyframe_cases as kc

NAMES = sorted(kc.CASES)
INT_OUTPUTS = {"view": ("ids", "nview", "cand", "ncand"), "pt": ("res",), "cma": ("out",), "tri": ("out",), "cmp": ("type", "comp")}
_memo = {}


def outputs(backend, name):
    key = (backend is numpy_ref, name)
    if key not in _memo:
        c = kc.CASES[name]
        _memo[key] = kc.run(backend, c.call, c.data)
    return _memo[key]


def point_in(call, data):
    return data[{"pt": "pts", "cma": "pts", "tri": "x3d"}[call]]


def point_out(call, o):
    return o[{"pt": "est", "cma": "pts", "tri": "x"}[call]]


def check_declared(c, o):
    """the declared output of a case against the outputs o of one implementation"""
    for k, w in c.want.items():
        if k == "moved":
            moved = (point_out(c.call, o) != point_in(c.call, c.data)).any(1)
            assert np.array_equal(moved, w), (c.name, "moved", moved)
        elif k == "z_side":
            assert np.sign(point_out(c.call, o)[0, 2] - point_in(c.call, c.data)[0, 2]) == w, (c.name, "z_side")
        elif k == "xzero":
            assert np.array_equal((o["x"] == 0).all(1), w), (c.name, "xzero", o["x"])
        elif k in ("c2p", "c2s"):
            assert np.array_equal(o[k], w), (c.name, k, o[k])
        else:
            assert np.array_equal(np.asarray(o[k]), np.asarray(w)), (c.name, k, o[k], w)


@pytest.mark.parametrize("name", NAMES)
def test_case_gives_declared_output(oracle, name):
    c = kc.CASES[name]
    o_orc, o_np = outputs(oracle, name), outputs(numpy_ref, name)
    check_declared(c, o_np)
    check_declared(c, o_orc)
    for k in INT_OUTPUTS[c.call]:
        assert np.array_equal(np.asarray(o_orc[k]), np.asarray(o_np[k])), (name, k)
    for k in set(o_orc) - set(INT_OUTPUTS[c.call]):  # points and chi2: the two implementations against each other
        np.testing.assert_allclose(o_orc[k], o_np[k], rtol=1e-8, atol=1e-9, err_msg="%s %s" % (name, k))


BANDED = [n for n in NAMES if kc.CASES[n].band]


@pytest.mark.parametrize("name", BANDED)
def test_banded_case_sits_in_its_band(oracle, name):
    b = kc.CASES[name].band
    q_np, q_orc = b["q"](numpy_ref), b["q"](oracle)
    assert q_np is not None
    assert kc.in_band(q_np, b["thr"], b["side"]), (name, q_np / b["thr"] - 1)
    if q_orc is not None:  # (a rejected triangulation returns no point to evaluate: the oracle is then held by its decision alone)
        assert kc.in_band(q_orc, b["thr"], b["side"]), (name, q_orc / b["thr"] - 1)
        assert abs(q_orc - q_np) <= 1e-8 * abs(q_np), (name, q_orc, q_np)


def test_banded_cases_come_in_both_sides():
    for n in BANDED:
        other = n.replace("_below", "_above") if n.endswith("_below") else n.replace("_above", "_below")
        assert other in kc.CASES and kc.CASES[other].band["side"] != kc.CASES[n].band["side"], n
    assert len(BANDED) >= 30 and len(BANDED) % 2 == 0


@pytest.mark.parametrize("a,b,out,elem", kc.PAIRS, ids=[p[0] + "|" + p[1] for p in kc.PAIRS])
def test_pairs_differ_in_the_declared_element(oracle, a, b, out, elem):
    for backend in (oracle, numpy_ref):
        oa, ob = outputs(backend, a), outputs(backend, b)
        ca, cb = kc.CASES[a], kc.CASES[b]
        assert ca.call == cb.call
        for k in INT_OUTPUTS[ca.call]:
            va, vb = np.atleast_1d(np.asarray(oa[k])).ravel(), np.atleast_1d(np.asarray(ob[k])).ravel()
            n = max(len(va), len(vb))  # (a view list is as long as its view: the shorter one is -1 padded, as the device pads it)
            va, vb = np.concatenate([va, -np.ones(n - len(va), va.dtype)]), np.concatenate([vb, -np.ones(n - len(vb), vb.dtype)])
            if k == out:
                assert va[elem] != vb[elem], (a, b, k)
                assert np.array_equal(np.delete(va, elem), np.delete(vb, elem)), (a, b, k, "another element differs too")
            elif k in kc.FOLLOWS.get(out, ()):
                assert not np.array_equal(va, vb), (a, b, k)
            else:
                assert np.array_equal(va, vb), (a, b, k)


def test_every_decision_has_two_sides():
    sides = {}
    for c in kc.CASES.values():
        sides.setdefault(c.decision, set()).add(c.side)
    assert set(sides) == set(kc.DECISIONS)
    for d in kc.DECISIONS:
        assert len(sides[d]) >= 2, (d, sides[d])


TIED = [n for n in NAMES if kc.CASES[n].tie]


@pytest.mark.parametrize("name", TIED)
def test_ties_are_bit_equal(name):
    a, b = kc.CASES[name].tie()
    assert a == b, (name, a, b)


CHECKED = [n for n in NAMES if kc.CASES[n].check]


@pytest.mark.parametrize("name", CHECKED)
def test_scene_assumptions_hold(name):
    c = kc.CASES[name]
    with kc.Ref(numpy_ref, c.data["mean"], c.data["cov"], c.data.get("prm")) as r:
        assert c.check(r, c.data), name


def test_tie_order_is_nanoflanns(oracle):
    """corr.tie: the order of bit-equal distances is that of the reference's own k-d tree, where the live build exists"""
    if not oracle.nf:  # (no skip: the confirmation is extra, the order itself is asserted by the cases; but say that it did not run)
        warnings.warn("oracle/_ref/libnanoflann_ref.so is absent: the tie order was not confirmed against nanoflann")
        return
    for name in ("corr_tie_k2", "corr_tie_k1", "corr_tie_at_kth"):
        c = kc.CASES[name]
        with kc.Ref(oracle, c.data["mean"], c.data["cov"]) as r:
            ids, m2, _, _ = r.view(c.data["cam"], c.data["pose"])
        idx = oracle.nanoflann_knn(np.ascontiguousarray(m2), c.data["uv"], c.data["k"])[0]
        assert np.array_equal(ids[np.asarray(idx).reshape(-1)[:c.data["k"]]], c.want["cand"][0]), name


@pytest.mark.parametrize("name", sorted(kc.REGIMES))
def test_regime_is_entered(oracle, name):
    r = kc.REGIMES[name]
    d = r["data"]
    with kc.Ref(numpy_ref, d["mean"], d["cov"]) as ref:
        ids, m2, c2, _ = ref.view(d["cam"], d["pose"])
    assert r["prop"](ids, m2, c2), r["why"]
    o_orc, o_np = kc.run(oracle, "view", d), kc.run(numpy_ref, "view", d)
    for k in INT_OUTPUTS["view"]:
        assert np.array_equal(np.asarray(o_orc[k]), np.asarray(o_np[k])), (name, k)


@pytest.mark.parametrize("name", sorted(kc.CHAINS))
def test_chain_case_gives_declared_output(oracle, name):
    ch = kc.CHAINS[name]
    for backend in (oracle, numpy_ref):
        for v, cand in zip(ch["views"], ch["cand"]):
            o = kc.run(backend, "view", v)
            assert np.array_equal(o["cand"], cand) and np.array_equal(o["ncand"], (cand >= 0).sum(1)), name
        o = kc.run(backend, ch["call"], ch["data"])  # (the data holds the tables the views give)
        for k, w in ch["want"].items():
            if k == "moved":
                assert np.array_equal((o["pts"] != ch["data"]["pts"]).any(1), w), name
            else:
                assert np.array_equal(o[k], w), (name, k, o[k])
