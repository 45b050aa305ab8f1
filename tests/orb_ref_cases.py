"""The cases whose outputs the reference's own ORB extractor gave, as recorded in tests/golden/golden_orb_ref.npz (tools/record_orb_ref.py
writes it from oracle/_ref/liborb_ref.so): the inputs, regenerated here from the hand-built cases of tests/orb_cases.py and from the seeded
scenes of tests/orb_scenes.py, and the reader of the recorded file.  tests/test_orb_ref_pin.py holds the model tests/orb_ref.py and the
declared expectations to it, tests/test_gpu_orb_ref.py the device.

A case: the keyword arguments of orb_ref.describe for one image, and `frame`: None, or (row_pad, lead) - the levels are then handed to the
reference (and to the device) as views into larger buffers, stride = width + row_pad, `lead` bytes in front.  The reference is given the
key-points that the call describes (orb_ref.live: deviations 1 and 2 are this project's notion; elsewhere the reference would index out of
range), compacted; `slots` maps them back.  A recorded result, per such key-point: angle f32 (computeOrientation's, run on EVERY one, also
where the case gives kp_angle), m_10 / m_01 i32 (what the reference handed to fastAtan2), ab (n, 2) f32 (the steering that the reference's
host computed for the angle the descriptor used: kp_angle where given, else `angle`), desc (n, 32) u8 (computeDescriptors on the level
blurred by orb_ref.blur - the blur is not the reference's - with that angle and the case's pattern).  The file holds these and the tables
umax and mvScaleFactor, and no pattern."""
import functools
import os

import numpy as np

from tests import orb_cases, orb_ref, orb_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "golden_orb_ref.npz")
FRAME = (13, 7)  # stride = width + 13, 7 bytes in front
SCENES = {"computed": dict(seed=7100), "computed_framed": dict(seed=7101, frame=FRAME), "given": dict(seed=7102, angles=True),
          "given_framed": dict(seed=7103, angles=True, frame=FRAME)}
SCENE_ARGS = dict(size=(160, 120), nlevels=4, n=300)
KEYS = ("angle", "m_10", "m_01", "ab", "desc")


def readonly(d):
    """(the arrays made here; the pattern is tests/orb_scenes.py's own object and stays as it is)"""
    for k, v in d.items():
        if k == "pattern":
            continue
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, list):
            for a in v:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scene(name, **over):
    """a random scene of the recorded geometry; `over`: other seeds for scenes that are not recorded (the live library's own pattern)"""
    kw = dict(SCENES[name], **over)
    frame = kw.pop("frame", None)
    return readonly(dict(orb_scenes.random_scene(**SCENE_ARGS, **kw), frame=frame))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, in the order of the recorded file"""
    out = {}
    for name, c in orb_cases.CASES.items():
        g = orb_cases.GROUPS[c["group"]]
        out["case/" + name] = dict(levels=c["levels"], kp_xy=c["kp_xy"], kp_oct=c["kp_oct"], pattern=g["pattern"], blur_w=g["blur_w"], scale_factor=1.2,
                                   n_kp=None, kp_angle=c["kp_angle"], frame=None)
    for name in SCENES:
        out["scene/" + name] = scene(name)
    return out


def slots(c):
    """the slots of a case that the call describes, ascending: the reference's key-point i is slot slots(c)[i]"""
    return np.array([i for i in range(len(c["kp_oct"])) if orb_ref.live(c["levels"], int(c["kp_xy"][i, 0]), int(c["kp_xy"][i, 1]), int(c["kp_oct"][i]))], np.int64)


def model_args(c):
    return {k: v for k, v in c.items() if k != "frame"}


def framed(img, frame):
    """the level as the reference gets it: itself, or a view into a larger buffer filled with 0xAB"""
    if frame is None:
        return np.ascontiguousarray(img)
    row_pad, lead = frame
    h, w = img.shape
    buf = np.full(lead + h * (w + row_pad), 0xAB, np.uint8)
    view = buf[lead:].reshape(h, w + row_pad)[:, :w]
    view[:] = img
    return view


def used_angle(c, r):
    """the angle that steers each described key-point's descriptor: kp_angle where the case gives it, else the reference's own"""
    return r["angle"] if c["kp_angle"] is None else np.asarray(c["kp_angle"], np.float32)[slots(c)]


def live_case(ref, c, pattern="case"):
    """one case through the live library `ref` (tests.oracle_lib.OrbRef).  pattern: "case" - the case's, or None - the extractor's own"""
    s = slots(c)
    n = len(s)
    r = dict(angle=np.zeros(n, np.float32), m_10=np.zeros(n, np.int32), m_01=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8))
    given = None if c["kp_angle"] is None else np.asarray(c["kp_angle"], np.float32)[s]
    for l in sorted(set(c["kp_oct"][s].tolist())):
        at = np.flatnonzero(c["kp_oct"][s] == l)
        xy = c["kp_xy"][s[at]]
        r["angle"][at], r["m_10"][at], r["m_01"][at] = ref.orientation(framed(c["levels"][l], c["frame"]), xy)
        blurred = framed(orb_ref.blur(c["levels"][l], c["blur_w"]), c["frame"])
        r["desc"][at] = ref.describe(blurred, xy, r["angle"][at] if given is None else given[at], c["pattern"] if pattern == "case" else None)
    r["ab"] = ref.steering(r["angle"] if given is None else given)
    return r


def live(ref):
    """every case through the live library -> ({name: result}, tables)"""
    return {name: live_case(ref, c) for name, c in cases().items()}, ref.tables()


def pack(results, tables):
    """{name: result} in the order of cases(), the tables -> the arrays of the file (data only)"""
    names = list(results)
    assert names == list(cases())
    cat = lambda key: np.concatenate([np.ascontiguousarray(results[n][key]) for n in names])
    return dict(names=np.array(names), n_kp=np.array([len(results[n]["angle"]) for n in names], np.int32), angle_bits=cat("angle").view(np.uint32),
                m_10=cat("m_10"), m_01=cat("m_01"), ab_bits=cat("ab").view(np.uint32), desc=cat("desc"),
                umax=np.asarray(tables["umax"], np.int32), scale_factor_bits=np.asarray(tables["scale_factor"], np.float32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def recorded():
    """the file -> ({name: result}, tables: umax, scale_factor); read-only arrays"""
    d = np.load(PATH)
    res, at = {}, 0
    for i, name in enumerate(d["names"].tolist()):
        n = int(d["n_kp"][i])
        sl = slice(at, at + n)
        res[name] = readonly(dict(angle=d["angle_bits"][sl].view(np.float32), m_10=d["m_10"][sl], m_01=d["m_01"][sl], ab=d["ab_bits"][sl].view(np.float32),
                                  desc=d["desc"][sl]))
        at += n
    assert at == len(d["angle_bits"]) == len(d["desc"])
    return res, readonly(dict(umax=d["umax"], scale_factor=d["scale_factor_bits"].view(np.float32)))


def record(ref):
    results, tables = live(ref)
    np.savez_compressed(PATH, **pack(results, tables))
    return results, tables


def ab_slots(c, r):
    """the reference's steering in the slots of the case (n, 2); 0 0 where the call describes nothing"""
    ab = np.zeros((len(c["kp_oct"]), 2), np.float32)
    ab[slots(c)] = r["ab"]
    return ab


def declared_steering(c, r):
    """per described key-point: the reference host's (a, b) ARE the declared steering of the angle its descriptor used"""
    want = np.array([orb_ref.steer(a) for a in used_angle(c, r)], np.float32).reshape(-1, 2)
    return (want.view(np.uint32) == np.ascontiguousarray(r["ab"]).view(np.uint32)).all(axis=1)


_model = {}


def model(name):
    """orb_ref.describe of a case under the declared steering, computed once per process and read-only"""
    if name not in _model:
        _model[name] = readonly(orb_ref.describe(**model_args(cases()[name])))
    return _model[name]


def as_outputs(c, r, declared):
    """what gl_orb_describe has to give for a case, from the reference's result r: `moments` and `angle` the reference's (0 0 and kp_angle
    where the case gives kp_angle), `desc` the reference's wherever its host's steering is the declared one and `declared`'s (the model
    under the declared steering) elsewhere, the rest `declared`'s (no arithmetic of the reference: the scaling and the counts)
    -> (outputs with the keys of tests.orb_dev.OUT_KEYS, the number of key-points whose descriptor is the model's)"""
    s = slots(c)
    out = {k: np.array(v) for k, v in declared.items()}
    same = declared_steering(c, r)
    out["desc"][s[same]] = r["desc"][same]
    out["angle"][s] = used_angle(c, r)
    if c["kp_angle"] is None:
        out["moments"][s] = np.stack([r["m_10"], r["m_01"]], 1)
    return out, int((~same).sum())
