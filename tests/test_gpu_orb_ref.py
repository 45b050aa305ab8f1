"""gl_orb_describe on the device against the reference's OWN ORB extractor: what oracle/_ref/liborb_ref.so gave for the cases and scenes
of tests/orb_ref_cases.py, as recorded in tests/golden/golden_orb_ref.npz (the reference tree itself is never read here), and the live
library as well where it has been built.  `moments` and `angle` equal the reference's bit for bit.  `desc` equals the reference's wherever
the reference host's (a, b) - libm's float cosine and sine - are the declared steering (the correctly rounded ones, include/gmmloc_hip.h);
elsewhere it equals the model's descriptor under the declared steering, and the test prints how many such key-points there were.  uv and
stat carry no arithmetic of the reference's half and are the model's.  Every run also checks the guard words behind the outputs and that
no input changed (tests/orb_dev.py)."""
import numpy as np
import pytest

from tests import oracle_lib, orb_dev, orb_ref
from tests import orb_ref_cases as RC
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu
NAMES = list(RC.cases())


@pytest.fixture(scope="module")
def live():
    """{name: result} of the live library where oracle/_ref/liborb_ref.so is present, else None"""
    ref = oracle_lib.load_orb_ref()
    return None if ref is None else RC.live(ref)[0]


def references(name, live):
    return [("recorded", RC.recorded()[0][name])] + ([("live", live[name])] if live is not None else [])


def device(gpu, cs, **kw):
    """cases of one pattern, blur, level shapes and framing as ONE call"""
    torch, ctx = gpu
    frame = cs[0]["frame"] or (0, 0)
    assert all(c["frame"] == cs[0]["frame"] for c in cs)
    return orb_dev.run(torch, ctx, cs, cs[0]["pattern"], cs[0]["blur_w"], cs[0]["scale_factor"], row_pad=frame[0], lead=frame[1], **kw)


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_reference(gpu, live, name):
    """B = 1: every hand-built case, and the four scenes of 160 x 120 with 4 levels and 300 key-points: orientation computed and given,
    levels tightly packed and with stride = width + 13 behind 7 leading bytes"""
    c = RC.cases()[name]
    got = device(gpu, [c])
    for what, r in references(name, live):
        want, by_model = RC.as_outputs(c, r, RC.model(name))
        print("%s (%s): %d of %d descriptors held to the model, not the reference (libm's steering is not the declared one)" %
              (name, what, by_model, len(RC.slots(c))))
        orb_dev.same_bits(got, orb_dev.expected([want], got["angle"].shape[1]), "%s (%s)" % (name, what))


def with_reference_angles(name):
    """the scene with the angles that the reference computed for it passed as kp_angle (0 where nothing is described)"""
    c, r = RC.cases()[name], RC.recorded()[0][name]
    assert c["kp_angle"] is None
    given = np.zeros(len(c["kp_oct"]), np.float32)
    given[RC.slots(c)] = r["angle"]
    return dict(c, kp_angle=given)


@pytest.mark.parametrize("pair", [("computed", "given"), ("computed_framed", "given_framed")], ids="+".join)
def test_batch_of_two_mixing_both_paths(gpu, live, pair):
    """B = 2 through kp_angle (one call has it for every image or for none): image 0 is the scene whose orientation the reference
    COMPUTED, passed with the reference's angles, image 1 the scene with GIVEN angles: the reference's descriptors of both, moments 0 0"""
    names = ["scene/" + p for p in pair]
    cs = [with_reference_angles(names[0]), RC.cases()[names[1]]]
    got = device(gpu, cs)
    declared = [orb_ref.describe(**RC.model_args(cs[0])), RC.model(names[1])]
    assert np.array_equal(declared[0]["desc"], RC.model(names[0])["desc"])  # (the same angles steer the same descriptors)
    for which in range(2 if live is not None else 1):
        wants = [RC.as_outputs(c, references(n, live)[which][1], d) for c, n, d in zip(cs, names, declared)]
        print("%s: %s descriptors held to the model" % (pair, [w[1] for w in wants]))
        assert not wants[0][0]["moments"].any() and not wants[1][0]["moments"].any()
        orb_dev.same_bits(got, orb_dev.expected([w[0] for w in wants], got["angle"].shape[1]), "B = 2 %s (%d)" % (pair, which))


def test_batch_of_two_computed(gpu, live):
    """B = 2 on the computed path, strided: the framed scene and the unframed one's content in the same framing"""
    names = ["scene/computed_framed", "scene/computed"]
    cs = [RC.cases()[names[0]], dict(RC.cases()[names[1]], frame=RC.FRAME)]  # (the framing is the caller's; the reference's answer does not depend on it)
    got = device(gpu, cs)
    for which in range(2 if live is not None else 1):
        wants = [RC.as_outputs(c, references(n, live)[which][1], RC.model(n)) for c, n in zip(cs, names)]
        orb_dev.same_bits(got, orb_dev.expected([w[0] for w in wants], got["angle"].shape[1]), "B = 2 computed (%d)" % which)


def test_the_extractors_own_pattern(gpu):
    """two random scenes described with the reference's OWN pattern, fetched from the live library at run time (the library ships
    none and the tests copy none): the device against the live reference, computed and given angles, strided"""
    ref = oracle_lib.load_orb_ref()
    if ref is None:
        pytest.skip("oracle/_ref/liborb_ref.so not built: the reference's own pattern is in no file of this project")
    t = ref.tables()
    assert t["npattern"] == 512 and np.abs(t["pattern"]).max() <= orb_ref.REACH
    own = t["pattern"].astype(np.int8)
    for name, seed in (("computed", 7200), ("given_framed", 7201)):
        c = dict(RC.scene(name, seed=seed), pattern=own)
        r = RC.live_case(ref, c, pattern=None)  # (None: the extractor's own vector, not the fetched copy)
        want, by_model = RC.as_outputs(c, r, orb_ref.describe(**RC.model_args(c)))
        print("own pattern, %s: %d of %d descriptors held to the model" % (name, by_model, len(RC.slots(c))))
        assert len(RC.slots(c)) >= 250 and len(np.unique(r["desc"], axis=0)) >= 200
        got = device(gpu, [c])
        orb_dev.same_bits(got, orb_dev.expected([want], got["angle"].shape[1]), "own pattern, " + name)
