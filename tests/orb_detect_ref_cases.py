"""The cases whose outputs the reference's own ORB extractor gave for its DETECTION half and for the whole detect(), as recorded in
tests/golden/golden_orb_detect_ref.npz (tools/record_orb_detect_ref.py writes it from oracle/_ref/liborb_ref.so, oracle/orb_detect_ref.cpp):
the inputs, regenerated here from seeds and from the hand-built cases of tests/orb_detect_cases.py, the runs through the live library, and
the reader of the recorded file.  tests/test_orb_detect_ref_pin.py holds the model tests/orb_detect_ref.py and the declared expectations to
it, tests/test_gpu_orb_detect_ref.py the device.

What the reference decides where its phase-2 sort (:664) sees two nodes of equal size is its allocator's choice (deviation 4 of
gl_orb_detect).  So every case here is asked of the MODEL first: `info["tie"]` of orb_detect_ref.distribute.  Tie-free cases are recorded
and compared in order; tied ones are never recorded - the pin enumerates their orders (the hand-built ones) or checks properties of the
live library's answer (at scale).  The file holds the reference's outputs only; no image, key set or pattern."""
import functools
import math
import os

import numpy as np

from tests import orb_detect_cases as HC
from tests import orb_detect_ref as M
from tests import orb_ref, orb_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "golden_orb_detect_ref.npz")
B = M.MIN_BORDER
f32 = np.float32


# ---- features per level: every nfeatures the constructor may be given up to 4 000
FPL = range(0, 4001)


# ---- the octree on seeded random key sets, tie-free by rejection ----------------------------------------------------------------------------
# draw(seed): the area by seed % 5 - 0, 1: 60 .. 200 x 60 .. 150 with nIni >= 1; 2: nIni = 2; 3: nIni = 3; 4: a strip taller than wide with
# nIni = 1.  2 .. 60 keys at distinct pixels in vToDistributeKeys' order (any order: the octree takes what it is given), responses 7 .. 120
# (repeats wanted: the final pick takes the first of equals), N = 2 .. 40.  The REJECTION RULE: a seed of OCT_SEEDS is kept iff the model
# reports no tie (no phase-2 sort saw two entries of equal size).  Nothing else is looked at; the counts that
# test_orb_detect_ref_pin.py asserts (64 / 32 / 32 and the nIni cover) are met by what this rule keeps.
OCT_SEEDS = range(0, 2600)


def n_ini_of(w, h):
    return int(math.floor(float(f32(w) / f32(h)) + 0.5))


def draw(seed):
    """-> (keys [(x, y, response)] relative to the borders, min_x, max_x, min_y, max_y, N)"""
    rng = np.random.default_rng(90000 + seed)
    kind = seed % 5
    while True:
        if kind <= 1:
            w, h = int(rng.integers(60, 201)), int(rng.integers(60, 151))
        elif kind == 4:
            w = int(rng.integers(40, 81))
            h = int(rng.integers(w + 1, 2 * w))
        else:
            h = int(rng.integers(36, 71))
            w = kind * h + int(rng.integers(-h // 3, h // 3 + 1))
        want = {2: 2, 3: 3, 4: 1}.get(kind)
        if n_ini_of(w, h) >= 1 and want in (None, n_ini_of(w, h)):
            break
    n = int(rng.integers(2, 61))
    cells = rng.choice(w * h, n, replace=False)
    keys = [(int(c % w), int(c // w), int(rng.integers(7, 121))) for c in cells]
    return keys, B, B + w, B, B + h, int(rng.integers(2, 41))


@functools.lru_cache(maxsize=None)
def octree_cases():
    """name -> dict(args: draw(seed), model: the model's vResultKeys, info) of every KEPT seed, in seed order"""
    out = {}
    for seed in OCT_SEEDS:
        args, info = draw(seed), {}
        res = M.distribute(*args, info=info)
        if not info["tie"]:
            out["oct/%d" % seed] = dict(args=args, model=res, info=info)
    return out


def in_input_order(keys, res):
    """the result's keys as the input has them, in input order"""
    chosen = set(res)
    return [k for k in keys if k in chosen]


# ---- the hand-built cases that reach DistributeOctTree ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_octree():
    """"<case>@<level>" -> dict(args, model, info, declared: the case's declared key-points of that level as (x, y, response) relative to
    the borders) for every level of every DETECT case that hands a non-empty key set to DistributeOctTree"""
    out = {}
    for name, c in HC.DETECT.items():
        for l, img in enumerate(c["levels"]):
            h, w = img.shape
            keys = M.candidates(img, c["ini_th"], c["min_th"])[0]
            if not keys or len(keys) > c["cand_cap"] or n_ini_of(w - 2 * B, h - 2 * B) < 1:
                continue
            n = M.features_per_level(c["nfeatures"], len(c["levels"]))[l]
            args, info = ([(x - B, y - B, s) for x, y, s in keys], B, w - B, B, h - B, n), {}
            res = M.distribute(*args, info=info)
            declared = [(x - B, y - B, r) for x, y, o, r in c["kp"] if o == l]
            out["%s@%d" % (name, l)] = dict(args=args, model=res, info=info, declared=declared)
    return out


ENUM_CAP = 512


def enumerate_orders(args, mut=(), cap=ENUM_CAP):
    """every answer the octree can give when each group of equal sizes that phase 2 reaches is walked in every order -> (the answers as
    a list of lists without repeats, whether the cap was hit)"""
    answers, stack, runs = [], [[]], 0
    while stack:
        prefix = stack.pop()
        info = {}
        res = M.distribute(*args, mut=mut, info=info, tie_order=prefix)
        runs += 1
        if res not in answers:
            answers.append(res)
        if runs >= cap:
            return answers, True
        for i in range(len(prefix), len(info["groups"])):
            for choice in range(1, math.factorial(info["groups"][i])):
                stack.append(prefix + [0] * (i - len(prefix)) + [choice])
    return answers, False


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def sparse(seed, size, dots):
    """a flat image (100) with `dots` single pixels of other values, each at least 20 px from every edge: sparse enough that small
    feature counts leave most levels without a tie"""
    rng = np.random.default_rng(91000 + seed)
    w, h = size
    img = np.full((h, w), 100, np.uint8)
    for _ in range(dots):
        x, y = int(rng.integers(20, w - 20)), int(rng.integers(20, h - 20))
        img[y, x] = int(np.clip(100 + rng.choice([-1, 1]) * rng.integers(9, 120), 0, 255))
    return img


def gap_scene(seed, dots, blobs, size=(256, 224)):
    """faint single pixels (8 .. 14 off the background: corners at min_th on levels 0 and 1, diluted below it by every further resize) and
    wide smooth blobs (amplitude 90, sigma 16 px: the centre of one falls by more than min_th within the ring's radius only once the blob
    is under 7.5 px wide, from level 5 on; a slope is no corner).  So the levels in between hold nothing: a level without key-points in
    FRONT of levels with some."""
    rng = np.random.default_rng(93000 + seed)
    w, h = size
    img = np.full((h, w), 100.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(blobs):
        cx, cy = rng.uniform(60, w - 60), rng.uniform(60, h - 60)
        img += 90.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 16.0 ** 2))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    for _ in range(dots):
        x, y = int(rng.integers(20, w - 20)), int(rng.integers(20, h - 20))
        img[y, x] = int(np.clip(int(img[y, x]) + rng.choice([-1, 1]) * rng.integers(8, 15), 0, 255))
    return img


def model_fast(level, x0, y0, view, threshold, nonmax):
    """the FAST callback answered by the model: orb_detect_ref.fast_cell on the cell image the reference passed, in its coordinates"""
    assert nonmax
    return M.fast_cell(view, 0, 0, view.shape[1], view.shape[0], threshold)


def model_blur(src, ksize, sigma):
    assert ksize == 7
    return orb_ref.blur(src, orb_ref.default_blur(sigma))


# the cell loop: name -> (levels, nfeatures of features_per_level, ini_th, min_th).  Single levels of 256 x 224, 92 x 92 and 752 x 480, the
# two geometries of orb_detect_cases.py whose last cell column (:775) / row (:767) is skipped, and two eight-level pyramids of sparse scenes
@functools.lru_cache(maxsize=None)
def cell_scenes():
    # (the single levels: a count at which the MODEL reports no tie, tried from 10 upwards; 2 000 is never reached, so phase 2 never starts
    # and every sweep runs)
    big = sparse(1, (256, 224), 120)
    out = {"256x224": ([big], 13, 20, 7), "256x224, count never reached": ([big], 2000, 20, 7), "92x92": ([sparse(2, (92, 92), 14)], 40, 20, 7),
           "752x480": ([sparse(3, (752, 480), 400)], 2000, 20, 7), "last column skipped 813x92": ([sparse(4, (813, 92), 60)], 100, 20, 7),
           "last row skipped 470x903": ([sparse(5, (470, 903), 300)], 13, 20, 7),
           "pyramid a": (M.pyramid(sparse(6, (256, 224), 150), 8), 40, 20, 7), "pyramid b": (M.pyramid(sparse(7, (256, 224), 220), 8), 40, 20, 7)}
    for name, c in HC.DETECT.items():  # every hand-built case whose levels have cells, with its own thresholds
        if all(min(l.shape) >= 62 and max(l.shape) <= 256 for l in c["levels"]) and c["mask"] == 0:
            out["case/" + name] = (c["levels"], c["nfeatures"], c["ini_th"], c["min_th"])
    for levels, *_ in out.values():
        for l in levels:
            l.setflags(write=False)
    return out


def expected_calls(levels, redo, ini_th=20, min_th=7):
    """the FAST record that cells() predicts: per level and cell {level, iniX, iniY, cols, rows, threshold, nonmax} at ini_th, and again
    at min_th where redo(level, cell index) says the first call came back empty"""
    out = []
    for l, img in enumerate(levels):
        for k, (_, _, x0, y0, x1, y1) in enumerate(M.cells(img.shape[1], img.shape[0])[2]):
            out.append((l, x0, y0, x1 - x0, y1 - y0, ini_th, 1))
            if redo(l, k):
                out.append((l, x0, y0, x1 - x0, y1 - y0, min_th, 1))
    return np.array(out, np.int32).reshape(-1, 7)


def model_redo(levels, ini_th, mut=()):
    """(level, cell index) -> the model's FAST finds nothing in that cell at ini_th (with "level_fallback": in no cell of the level)"""
    empty = {(l, k): not M.fast_cell(img, x0, y0, x1, y1, ini_th) for l, img in enumerate(levels)
             for k, (_, _, x0, y0, x1, y1) in enumerate(M.cells(img.shape[1], img.shape[0])[2])}
    if "level_fallback" in mut:
        return lambda l, k: all(v for (ll, _), v in empty.items() if ll == l)
    return lambda l, k: empty[(l, k)]


def script(levels):
    """scripted answers of the FAST callback: (level, cell index) -> (threshold at which the cell answers, [(x, y, response)] in the cell
    image's coordinates).  Every third cell answers at 20, every third only at 7, the rest never; an answering cell returns its first
    computed pixel (3, 3), its last (cols - 4, rows - 4) and one between, all of one response - so the final pick of a node shows the
    ORDER in which the keys arrived (the first of equals)."""
    out = {}
    for l, img in enumerate(levels):
        for k, (_, _, x0, y0, x1, y1) in enumerate(M.cells(img.shape[1], img.shape[0])[2]):
            cols, rows = x1 - x0, y1 - y0
            if k % 3 < 2 and cols >= 8 and rows >= 8:
                out[(l, k)] = ((20, 7)[k % 3], [(3, 3, 50), (cols - 4, rows - 4, 50), (3 + (cols - 7) // 2, 3 + (rows - 7) // 2, 50)])
    return out


def scripted_candidates(levels):
    """what candidates() says the scripted answers become: shifted by the cell's origin (j wCell, i hCell), cells in order -> per level
    [(x, y, response)] relative to the borders"""
    sc, out = script(levels), []
    for l, img in enumerate(levels):
        keys = []
        for k, (_, _, x0, y0, _, _) in enumerate(M.cells(img.shape[1], img.shape[0])[2]):
            keys += [(x + x0 - B, y + y0 - B, r) for x, y, r in sc.get((l, k), (0, []))[1]]
        out.append(keys)
    return out


def scripted_model(levels, per_level):
    """the model's octree on the scripted candidates -> ((n, 6) key-points as the reference returns them without the angle, tie per level)"""
    rows, tie = [], []
    sf = orb_ref.scale_table(1.2)
    for l, (img, keys) in enumerate(zip(levels, scripted_candidates(levels))):
        info = {}
        res = M.distribute(keys, B, img.shape[1] - B, B, img.shape[0] - B, per_level[l], info=info) if keys else []
        tie.append(info.get("tie", False))
        rows += [(x + B, y + B, l, int(f32(31) * sf[l]), r) for x, y, r in res]
    return np.array(rows, np.float32).reshape(-1, 5), tie


def model_key_points(levels, nfeatures, ini_th, min_th, mut=()):
    """the model's detect() as ComputeKeyPointsOctTree returns allKeypoints: (n, 6) f32 {x, y, octave, size, response, angle}, the angle
    orb_ref.ic_angle's, size = (int)(PATCH_SIZE * mvScaleFactor[level]) (:809) -> (key-points, the model's detect dict)"""
    m = M.detect(levels, nfeatures, 1.2, ini_th, min_th, mut=mut)
    sf = orb_ref.scale_table(1.2)
    kp = np.zeros((len(m["kp_oct"]), 6), np.float32)
    for i, ((x, y), l, r) in enumerate(zip(m["kp_xy"], m["kp_oct"], m["kp_response"])):
        kp[i] = (x, y, l, int(f32(31) * sf[l]), r, orb_ref.ic_angle(levels[l], int(x), int(y))[2])
    return kp, m


def tie_free_rows(kp, tie):
    """the key-point rows of the levels that the model calls tie-free"""
    keep = np.array([not tie[int(l)] for l in kp[:, 2]], bool).reshape(-1)
    return kp[keep]


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------------------
def near_half(n, levels=8):
    """(float)n * inv[l] lies on a half or within two floats of one at some level 1 .. levels - 1"""
    sf = orb_ref.scale_table(1.2)
    for l in range(1, levels):
        v = f32(n) * (f32(1.0) / sf[l])
        frac = float(v) - math.floor(float(v))
        if abs(frac - 0.5) <= 2 * float(np.spacing(v)):
            return True
    return False


@functools.lru_cache(maxsize=None)
def pyramid_sizes():
    """>= 20 (width, height) pairs: the sizes the project runs, and pairs from the search for a level size on or next to a half (found
    among 20 .. 1 300; each such number is used as a width and as a height beside a small other side)"""
    special = [n for n in range(20, 1300) if near_half(n)]
    pairs = [(752, 480), (640, 480), (256, 224), (161, 119), (125, 75), (100, 101), (63, 63), (45, 45)]
    for i, n in enumerate(special[:16]):
        pairs.append((n, 40 + i) if i % 2 == 0 else (40 + i, n))
    return special, pairs


def pyramid_image(w, h):
    rng = np.random.default_rng(92000 + 4096 * w + h)
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


PYRAMID_PIXELS = [(256, 224), (161, 119), (45, 45)]  # the pairs whose levels are compared pixel by pixel and whose borders are overwritten


# ---- the whole detect() --------------------------------------------------------------------------------------------------------------------
# two gap scenes of 256 x 224, 8 levels: (seed, dots, blobs, nfeatures), found by trying seeds 0 .. 5 at nfeatures 30, 40, 60, 80 and keeping
# what the MODEL calls tie-free on every level with a phase-2 sort on some, and with a level without key-points in front of a level with
# some.  test_orb_detect_ref_pin.py asserts all three on the model.
DETECT_SCENES = {"detect a": (3, 120, 6, 40), "detect b": (5, 90, 5, 60)}


@functools.lru_cache(maxsize=None)
def detect_scene(name):
    seed, dots, blobs, nfeatures = DETECT_SCENES[name]
    img = gap_scene(seed, dots, blobs)
    img.setflags(write=False)
    return img, nfeatures


@functools.lru_cache(maxsize=None)
def detect_model(name):
    """the two models chained up to the angle: (levels, orb_detect_ref.detect's dict)"""
    img, nfeatures = detect_scene(name)
    levels = M.pyramid(img, 8)
    return levels, M.detect(levels, nfeatures)


# ---- the runs through the live library -----------------------------------------------------------------------------------------------------
def live(ref):
    """every recorded quantity from the live library `ref` (tests.oracle_lib.OrbRef) -> {key: array}; lists of arrays are stored as a
    count array and their concatenation (pack / unpack)"""
    out = {"fpl": np.array([ref.features_per_level(n) for n in FPL], np.int16)}
    out.update(pack("oct", [np.array(ref.distribute(*c["args"]), np.int32).reshape(-1, 3) for c in octree_cases().values()]))
    hand = [(n, c) for n, c in hand_octree().items() if not c["info"]["tie"]]
    out.update(pack("hand", [np.array(ref.distribute(*c["args"]), np.int32).reshape(-1, 3) for _, c in hand]))
    out["hand_names"] = np.array([n for n, _ in hand])
    # the cell loop: the FAST record with a callback that finds nothing, the scripted key-points, the model's FAST
    names = list(cell_scenes())
    lists = {k: [] for k in ("cell_empty_calls", "cell_all_kp", "cell_all_calls", "cell_one_kp", "cell_one_calls", "cell_fast_kp", "cell_fast_calls")}
    for name in names:
        levels, nfeatures, ini_th, min_th = cell_scenes()[name]
        lists["cell_empty_calls"].append(live_cells(ref, levels, [nfeatures] * len(levels), None)[1])
        for n, which in ((SCRIPT_ALL, "all"), (1, "one")):
            kp, calls = live_cells(ref, levels, [n] * len(levels), script(levels))
            lists["cell_%s_kp" % which].append(tie_free_rows(kp, scripted_model(levels, [n] * len(levels))[1]))
            lists["cell_%s_calls" % which].append(calls)
        kp, calls = live_fast(ref, levels, nfeatures, ini_th, min_th)
        lists["cell_fast_kp"].append(tie_free_rows(kp, M.detect(levels, nfeatures, 1.2, ini_th, min_th)["tie"]))
        lists["cell_fast_calls"].append(calls)
    out["cell_names"] = np.array(names)
    for k, v in lists.items():
        out.update(pack(k, v))
    # the pyramid
    sizes, pixels = [], []
    for w, h in pyramid_sizes()[1]:
        lv = live_pyramid(ref, pyramid_image(w, h))[0]
        sizes.append(np.array([l["shape"] + (l["step"], l["offset"], l["store"]) for l in lv], np.int32))
        if (w, h) in PYRAMID_PIXELS:
            pixels += [l["pixels"].reshape(-1) for l in lv]
    out.update(pack("pyr", sizes))
    out.update(pack("pyr_px", pixels))
    # detect()
    det = [live_detect(ref, *detect_scene(name)) for name in DETECT_SCENES]
    out.update(pack("detect_kp", [d[0] for d in det]))
    out.update(pack("detect_desc", [d[1] for d in det]))
    out.update(pack("detect_ab", [ref.steering(d[0][:, 5]) for d in det]))  # (a, b) as the recording host's libm steered each descriptor
    # computeDescriptors once more on detect()'s own key-points and angles, with a pattern this project holds (orb_scenes.PATTERN): what
    # the device can be held to where the extractor's own pattern is not at hand
    again = []
    for name, (kp, _) in zip(DETECT_SCENES, det):
        levels, m = detect_model(name)
        desc = np.zeros((len(kp), 32), np.uint8)
        for l in sorted(set(m["kp_oct"].tolist())):
            at = np.flatnonzero(m["kp_oct"] == l)
            desc[at] = ref.describe(model_blur(levels[l], 7, 2.0), m["kp_xy"][at], kp[at, 5], orb_scenes.PATTERN)
        again.append(desc)
    out.update(pack("detect_desc_pat", again))
    return out


SCRIPT_ALL = 10000  # a per-level count that no stop test reaches: every scripted key-point comes out, and phase 2 never starts


def live_fast(ref, levels, nfeatures, ini_th, min_th):
    """ComputeKeyPointsOctTree on caller levels with the FAST callback answered by the model's fast_cell -> (key-points, record)"""
    ref.set_hooks(fast=model_fast)
    ref.set_levels(levels, M.features_per_level(nfeatures, len(levels)), ini_th, min_th)
    ref.fast_calls()
    kp = ref.key_points()[1]
    return kp, ref.fast_calls()


def live_cells(ref, levels, per_level, scripted, ini_th=20, min_th=7):
    """ComputeKeyPointsOctTree on caller levels with the FAST callback answering from `scripted` (None: nothing) -> (key-points, record)"""
    cell_of = {}
    for l, img in enumerate(levels):
        for k, (_, _, x0, y0, _, _) in enumerate(M.cells(img.shape[1], img.shape[0])[2]):
            cell_of[(l, x0, y0)] = k

    def fast(level, x0, y0, view, threshold, nonmax):
        th, keys = (scripted or {}).get((level, cell_of[(level, x0, y0)]), (0, []))
        return keys if threshold == th else []

    ref.set_hooks(fast=fast)
    ref.set_levels(levels, per_level, ini_th, min_th)
    ref.fast_calls()
    kp = ref.key_points()[1]
    return kp, ref.fast_calls()


def live_pyramid(ref, image, nfeatures=40):
    """ComputePyramid with cv::resize answered by the model's resize -> (the levels as OrbRef.pyramid gives them, the hand-overs: per
    resize call (the source as the reference passed it, the destination's shape))"""
    seen = []

    def resize(src, shape):
        seen.append((src.copy(), shape))
        return M.resize(src, shape)

    ref.set_hooks(fast=model_fast, resize=resize, blur=model_blur)
    return ref.pyramid(image, nfeatures), seen


def live_detect(ref, image, nfeatures):
    ref.set_hooks(fast=model_fast, resize=M.resize, blur=model_blur)
    return ref.detect(image, nfeatures)


def pack(key, arrays):
    """a list of arrays of one dtype and trailing shape -> {key + "_n": leading lengths, key: the concatenation}"""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    return {key + "_n": np.array([len(a) for a in arrays], np.int32), key: np.concatenate(arrays) if arrays else np.zeros(0, np.int32)}


def unpack(d, key):
    at, out = 0, []
    for n in d[key + "_n"].tolist():
        out.append(d[key][at:at + n])
        at += n
    assert at == len(d[key]), key
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    d = np.load(PATH)
    out = {k: d[k] for k in d.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def record(ref):
    res = live(ref)
    np.savez_compressed(PATH, **res)
    return res
