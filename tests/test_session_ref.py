"""CPU: the mapping session of tests/session_ref.py on the model leg alone, its float producers the C++ oracle and the numpy restatements
the per-call *_ref tests use.  The oracle's floats differ from the device's inside the known tolerances, so nothing here is compared with
the device's session; this file shows that
  - every invariant of session_ref.check_state holds on the model after every step of every key-frame (and that check_state notices
    each of them broken);
  - the session is what it was built to be: every event tests/test_gpu_session.py relies on happens at least once over the four
    key-frames, the events that floats decide at least session_ref.CPU_REACHED times;
  - the models compose: their own consistency checks pass on what every step leaves (Host.take), the object model of the graph and its
    row representation agree after every edit (Host.graph_agrees), gl_map_stats_track stated directly agrees with the model's (m_track)."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import session_ref as SR
from tests import session_scenes as SS


@pytest.fixture(scope="module")
def session(oracle, map_v1, gt_sync):
    mean, cov = map_v1
    P = SR.OracleProducers(oracle, api.Camera(), mean, cov)
    sc = SS.session_scene(mean, cov, gt_sync["V1_01_easy"], P.search2d)
    states = []
    out, H, entry = SR.model_leg(sc, P, check=lambda s, K, name: states.append((K, name)) or SR.check_state(s, (K, name)))
    P.close()
    assert len(states) == len(sc["arrivals"]) * len(SR.STEPS)
    return sc, out, H, entry


def test_invariants_hold_on_the_model_after_every_step(session):
    sc, out, H, entry = session  # (model_leg has run check_state after every step: a broken invariant fails the fixture)
    SR.check_state(entry, "entry")
    assert list(out) == [(K, name) for K in sc["arrivals"] for name in SR.STEPS]


def test_the_session_is_what_it_was_built_to_be(session):
    sc, out, H, entry = session
    print("events", dict(H.events), "needs", dict(H.need))
    for k in SR.EVENTS:
        assert H.events[k] >= SR.CPU_REACHED.get(k, 1), (k, H.events[k])
    ev = SR.events_of_results(out)  # (the same events counted from the step results alone, as the GPU test counts the device leg's)
    for k in ev:
        assert ev[k] == H.events[k], (k, ev[k], H.events[k])
    assert sc["m"]["kf_mp"].shape == (20, 140) and 1500 < len(sc["m"]["mp_valid"]) < 2000


def test_the_candidate_list_carries_over(session):
    """removeMapPoints judges entries a second time that an earlier key-frame kept, and meets rows that died in between"""
    sc, out, H, entry = session
    assert H.events["kept_met_again"] >= 1 and H.events["invalid"] >= 1 and H.events["ratio"] >= 1 and H.events["young_few"] >= 1 and H.events["aged"] >= 1


def test_the_composites_read_fresh_lists_where_the_reference_reads_stored_ones(session):
    """the declared deviation of session_ref's docstring, counted: how often the stored list and the fresh count differed in this session"""
    sc, out, H, entry = session
    print("stored list != fresh count: createMapPoints %d of %d key-frames, removeKeyFrames %d of %d" %
          (H.events["stale_nn_list"], len(sc["arrivals"]), H.events["stale_cull_list"], len(sc["arrivals"])))


def _broken(s, **kw):
    t = {k: np.array(v) for k, v in s.items()}
    for k, f in kw.items():
        f(t[k])
    return t


def test_check_state_notices_each_break(session):
    sc, out, H, entry = session
    s = out[(sc["arrivals"][-1], SR.STEPS[-1])][0]
    SR.check_state(s)
    p = int(np.nonzero((s["mp_valid"] != 0) & (np.diff(s["obs_ptr"]) >= 2))[0][0])
    o = int(s["obs_ptr"][p])
    dead_kf = int(np.nonzero(s["kf_valid"] == 0)[0][-1])
    row = int(np.argmax(s["cov_n"]))

    def bump_ptr(a):
        a[-1] += 1

    def name_dead(a):
        a[o] = dead_kf

    def twice(a):
        a[o + 1] = a[o]

    def other_slot(a):
        a[s["obs_kf"][o], s["obs_feat"][o]] = -1

    def kill(a):
        a[p] = 0

    def stale_ref(a):
        a[p] = dead_kf

    def found_more(a):
        a[p] = s["visible"][p] + 1

    def cycle(a):
        a[p], a[p + 1] = p + 1, p

    def unsorted(a):
        a[row, 0], a[row, 1] = a[row, 1] - 1, a[row, 0] + 1

    def short_prefix(a):
        a[row] = s["cov_n"][row] + 1

    def cand_out(a):
        a[0] = len(s["mp_valid"])

    for key, f in (("obs_ptr", bump_ptr), ("obs_kf", name_dead), ("obs_kf", twice), ("kf_mp", other_slot), ("mp_valid", kill), ("mp_ref_kf", stale_ref),
                   ("found", found_more), ("mp_replaced", cycle), ("cov_w", unsorted), ("cov_nord", short_prefix), ("cand", cand_out)):
        with pytest.raises(AssertionError):
            SR.check_state(_broken(s, **{key: f}), f.__name__)
