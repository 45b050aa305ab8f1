"""The model of gl_orb_describe (tests/orb_ref.py) and the declared expectations of tests/orb_cases.py against the reference's OWN ORB
extractor, on the CPU: what oracle/_ref/liborb_ref.so gave (gmmloc/src/cv/orb_extractor.cpp compiled where it lies against this project's
OpenCV stand-in, oracle/orb_ref.cpp), as recorded in tests/golden/golden_orb_ref.npz.  Every comparison is exact.  The tests on the
recorded file never skip; where the library is built it is run as well (the tests named or parametrised `live`).

What is the reference's here: the constructor's tables, the traversal of the patch and the moments, the order of fastAtan2's arguments,
the steered read, cvRound's place in it, the comparison, the bit order - and the OVERLOAD of cos / sin, which is libm's cosf / sinf: the
last bit of (a, b) is the recording host's libm's choice, so every descriptor is compared with the model under the reference's own (a, b),
and with the model under the declared steering (the correctly rounded cosine and sine) wherever the two steerings are the same floats.
What is NOT the reference's: the polynomial of fastAtan2 (the stand-in's, this project's statement) and the blur (the caller's)."""
import numpy as np
import pytest

from tests import oracle_lib, orb_cases, orb_ref
from tests import orb_ref_cases as RC

f32 = np.float32
NAMES = list(RC.cases())
SOURCES = ["recorded", "live"]
_live = {}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def source(which):
    """({name: result}, tables) of the recorded file, or of the live library run once (skips where it is not built)"""
    if which == "recorded":
        return RC.recorded()
    ref = oracle_lib.load_orb_ref()
    if ref is None:
        pytest.skip("oracle/_ref/liborb_ref.so not built")
    if "all" not in _live:
        _live["all"] = RC.live(ref)
    return _live["all"]


def test_the_file_holds_every_case_and_no_pattern():
    rec, tables = RC.recorded()
    assert list(rec) == NAMES
    stored = np.load(RC.PATH)
    assert sorted(stored.files) == sorted(["names", "n_kp", "angle_bits", "m_10", "m_01", "ab_bits", "desc", "umax", "scale_factor_bits"])
    for name, c in RC.cases().items():
        n = len(RC.slots(c))
        assert all(len(rec[name][k]) == n for k in RC.KEYS), name
    scenes = [RC.cases()["scene/" + s] for s in RC.SCENES]
    assert all(len(RC.slots(c)) >= 250 and len(set(c["kp_oct"][RC.slots(c)].tolist())) == 4 for c in scenes)
    assert sum(c["frame"] is not None for c in scenes) >= 1 and {c["kp_angle"] is None for c in scenes} == {True, False}


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SOURCES)
def test_tables(which):
    """umax as the constructor leaves it; mvScaleFactor bit for bit: a float times the DOUBLE member scaleFactor, not init_config.hpp's
    float table"""
    tables = source(which)[1]
    assert tables["umax"].tolist() == orb_ref.UMAX == orb_cases.UMAX
    assert bits_equal(np.asarray(tables["scale_factor"], f32), orb_ref.scale_table(1.2))
    assert bits_equal(np.asarray(tables["scale_factor"], f32), np.array(orb_cases.SF, f32))


def test_the_extractors_own_pattern_is_never_refused():
    """live only: 512 entries, all within [-13, 13] - deviation 3 never refuses the pattern a host passes"""
    t = source("live")[1]
    assert t["npattern"] == 512 and np.abs(t["pattern"]).max() <= orb_ref.REACH
    assert len(np.unique(t["pattern"], axis=0)) > 200  # (a table, not a constant)


# ---- moments and angle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SOURCES)
def test_moments_and_angle(which):
    """every described key-point of every case and scene: the moments the reference hands to fastAtan2 == orb_ref.ic_angle's, and the
    declared ones where a case declares them; its angle bits == orb_ref.fast_atan2(m_01, m_10).  The angle shows the ORDER of the
    arguments and the traversal only: the polynomial behind it is the stand-in's, written by this project from the header's rule, and
    proves nothing about OpenCV's.  Views with stride above width and a leading offset included."""
    res = source(which)[0]
    total = 0
    for name, c in RC.cases().items():
        r, s = res[name], RC.slots(c)
        for i, slot in enumerate(s):
            x, y, l = int(c["kp_xy"][slot, 0]), int(c["kp_xy"][slot, 1]), int(c["kp_oct"][slot])
            m_10, m_01, angle = orb_ref.ic_angle(c["levels"][l], x, y)
            assert (int(r["m_10"][i]), int(r["m_01"][i])) == (m_10, m_01), (name, slot)
            assert bits_equal(r["angle"][i], angle), (name, slot, r["angle"][i], angle)
            assert bits_equal(r["angle"][i], orb_ref.fast_atan2(f32(r["m_01"][i]), f32(r["m_10"][i])))
        if name.startswith("case/") and c["kp_angle"] is None:
            e = orb_cases.CASES[name[5:]]["expect"]
            assert bits_equal(np.stack([r["m_10"], r["m_01"]], 1), e["moments"][s]), name
            exact = ~np.isnan(e["angle"][s])
            assert bits_equal(r["angle"][exact], e["angle"][s][exact]), name
        if c["kp_angle"] is None:
            m = RC.model(name)
            assert bits_equal(m["moments"][s], np.stack([r["m_10"], r["m_01"]], 1)) and bits_equal(m["angle"][s], r["angle"]), name
        total += len(s)
    assert total >= 1200


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SOURCES)
def test_steering_is_libms_float_cosine_within_one_ulp_of_the_declared(which):
    """the reference host's (a, b) are the declared steering or its neighbouring float: the float overload, whose last bit is libm's"""
    res = source(which)[0]
    off = n = 0
    for name, c in RC.cases().items():
        r = res[name]
        want = np.array([orb_ref.steer(a) for a in RC.used_angle(c, r)], f32).reshape(-1, 2)
        up, down = np.nextafter(want, f32(np.inf)), np.nextafter(want, f32(-np.inf))
        assert ((r["ab"] == want) | (r["ab"] == up) | (r["ab"] == down)).all(), name
        off += int((~RC.declared_steering(c, r)).sum())
        n += len(want)
    print("%s: %d of %d key-points steered by an (a, b) other than the correctly rounded one" % (which, off, n))


def check_descriptors(name, r):
    """EVERY key-point: the reference's descriptor == the model's under the reference host's (a, b); == the model's under the declared
    steering wherever (a, b) are the declared ones; the declared byte where a case declares it.  No key-point is set aside."""
    c = RC.cases()[name]
    s = RC.slots(c)
    under_ref = orb_ref.describe(**RC.model_args(c), ab=RC.ab_slots(c, r))
    assert bits_equal(under_ref["desc"][s], r["desc"]), (name, np.flatnonzero((under_ref["desc"][s] != r["desc"]).any(axis=1)))
    same = RC.declared_steering(c, r)
    declared = RC.model(name)
    assert bits_equal(declared["desc"][s][same], r["desc"][same]), name
    if name.startswith("case/"):
        e = orb_cases.CASES[name[5:]]["expect"]
        assert bits_equal(e["desc"][s][same], r["desc"][same]), name


@pytest.mark.parametrize("name", NAMES)
def test_descriptors(name):
    check_descriptors(name, RC.recorded()[0][name])


def test_descriptors_live():
    res = source("live")[0]
    for name in NAMES:
        check_descriptors(name, res[name])


# ---- mutations ------------------------------------------------------------------------------------------------------------------------------
# rules of the model that the pinned functions do not run, exempt by name, each with the reason
NOT_PINNED = {"reflect": "the blur's border rule: the blur is the caller's, OpenCV's GaussianBlur is not run",
              "blur_round": "the blur's rounding constant: the blur is the caller's, OpenCV's GaussianBlur is not run"}
PINNED = [rule for rule in orb_ref.MUTATIONS if rule not in NOT_PINNED]
assert len(PINNED) == len(orb_ref.MUTATIONS) - 2 == 5 + 32


def contradicted(rule, c, r):
    """the model with `rule` swapped for its neighbour, under the reference's own (a, b), disagrees with the reference on this case"""
    s = RC.slots(c)
    m = orb_ref.describe(**RC.model_args(c), ab=RC.ab_slots(c, r), mut=(rule,))
    if c["kp_angle"] is None and not (bits_equal(m["moments"][s], np.stack([r["m_10"], r["m_01"]], 1)) and bits_equal(m["angle"][s], r["angle"])):
        return True
    return not bits_equal(m["desc"][s], r["desc"])


def check_rule(rule, res):
    seen = next((name for name, c in RC.cases().items() if name.startswith("case/") and contradicted(rule, c, res[name])), None)
    assert seen is not None, "the reference contradicts the rule %s on no case" % rule


@pytest.mark.parametrize("rule", PINNED)
def test_the_reference_contradicts_each_neighbouring_rule(rule):
    """half_away, moments_blurred, le, swap_row_col, every umax +-1 @ v, and contract (the recorded build is -ffp-contract=off): the
    reference itself says no to each on at least one hand-built case"""
    check_rule(rule, RC.recorded()[0])


def test_the_live_reference_contradicts_each_neighbouring_rule():
    res = source("live")[0]
    for rule in PINNED:
        check_rule(rule, res)


# ---- the outputs that do not depend on libm ------------------------------------------------------------------------------------------------
def test_live_and_recorded_agree_where_libm_has_no_say():
    """tables, moments and angles: bit for bit.  Descriptors and (a, b) are held to the model each under its own (a, b) above, not to
    each other: another glibc may round cosf / sinf differently."""
    (live, ltab), (rec, rtab) = source("live"), RC.recorded()
    assert bits_equal(ltab["umax"], rtab["umax"]) and bits_equal(ltab["scale_factor"], rtab["scale_factor"])
    assert list(live) == list(rec)
    for name in rec:
        for k in ("m_10", "m_01", "angle"):
            assert bits_equal(live[name][k], rec[name][k]), (name, k)
