"""The model of gl_orb_pyramid / gl_orb_detect (tests/orb_detect_ref.py) and the declared expectations of tests/orb_detect_cases.py against
the reference's OWN ORB extractor, on the CPU: what oracle/_ref/liborb_ref.so gave (gmmloc/src/cv/orb_extractor.cpp compiled where it lies
against this project's OpenCV stand-in; oracle/orb_detect_ref.cpp), as recorded in tests/golden/golden_orb_detect_ref.npz.  Every comparison
is exact.  The tests on the recorded file never skip; where the library is built it is run as well (the tests parametrised or named
`live`; without it they skip).

What is the reference's here: the constructor's mnFeaturesPerLevel; ComputePyramid's sizes, hand-over from level to level and views; the
cell loop of ComputeKeyPointsOctTree - rectangles, order, the two `continue`s, the per-cell fallback, the shift into the level;
DistributeOctTree and DivideNode - the float node edges, the list order, the three stop tests, phase 2; computeOrientation behind them; and
detect()'s order, scaling and descriptors.  Where a phase-2 sort sees two nodes of EQUAL SIZE the reference sorts node addresses: its
answer is its allocator's and differs between two runs of one binary.  Such cases are never compared in order: the hand-built ones are
enumerated over every order, the ones at scale are checked for properties only.

What is NOT the reference's and stays declared: cv::FAST (the segment test, the score, the suppression: the model's swapped rules `arc8`,
`arc10`, `ge`, `score_off`, `nonstrict`, `nms_across`), cv::resize (`no_shift4`) and cvRound (`half_up`).  The stand-in hands FAST and
resize to the model itself and rounds as this project declares, so no run here can contradict them: OpenCV is not at hand."""
import functools

import numpy as np
import pytest

from tests import oracle_lib, orb_ref, orb_scenes
from tests import orb_detect_cases as HC
from tests import orb_detect_dev as dev
from tests import orb_detect_ref as M
from tests import orb_detect_ref_cases as RC

SOURCES = ["recorded", "live"]
B = M.MIN_BORDER
_live = {}


def library():
    ref = oracle_lib.load_orb_ref()
    if ref is None or not ref._detect_half:
        pytest.skip("oracle/_ref/liborb_ref.so not built")
    return ref


def source(which):
    """{key: array} of the recorded file, or of the live library run once"""
    if which == "recorded":
        return RC.recorded()
    ref = library()
    if "all" not in _live:
        _live["all"] = RC.live(ref)
    return _live["all"]


def rows(a):
    return [tuple(int(v) for v in r) for r in a]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_file_holds_the_references_outputs_only():
    d = RC.recorded()
    assert sorted(k for k in d if not k.endswith("_n")) == sorted(
        ["fpl", "oct", "hand", "hand_names", "cell_names", "cell_empty_calls", "cell_all_kp", "cell_all_calls", "cell_one_kp", "cell_one_calls",
         "cell_fast_kp", "cell_fast_calls", "pyr", "pyr_px", "detect_kp", "detect_desc", "detect_ab", "detect_desc_pat"])
    assert d["cell_names"].tolist() == list(RC.cell_scenes()) and len(d["oct_n"]) == len(RC.octree_cases())
    assert d["hand_names"].tolist() == [n for n, c in RC.hand_octree().items() if not c["info"]["tie"]]  # no tied case is recorded


# ---- features per level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SOURCES)
def test_features_per_level(which):
    """mnFeaturesPerLevel of a constructed extractor (8 levels, 1.2) for EVERY nfeatures from 0 to 4 000"""
    got = source(which)["fpl"]
    assert got.shape == (4001, 8)
    for n in RC.FPL:
        assert got[n].tolist() == M.features_per_level(n, 8), n


# ---- the octree, tie-free ---------------------------------------------------------------------------------------------------------------------
def test_the_model_alone_meets_the_case_counts():
    """what the rejection rule keeps: >= 64 cases whose phase 2 sorted two or more entries, walked more than one node and left the keys
    in another order than they came in; >= 32 that end in phase 1 by size == prevSize; >= 32 that end by size >= N at the first sweep;
    nIni = 1, 2, 3; strips taller than wide"""
    oc = RC.octree_cases()
    assert not any(c["info"]["tie"] for c in oc.values())
    phase2 = [c for c in oc.values() if c["info"]["sorts"] >= 1 and c["info"]["walked"] >= 2 and c["model"] != RC.in_input_order(c["args"][0], c["model"])]
    assert len(phase2) >= 64, len(phase2)
    assert all(M.distribute(*c["args"], mut=("tie_rev",)) == c["model"] for c in phase2)  # tie-free: the declared order has no say
    assert sum(c["info"]["end"] == "sweep same" for c in oc.values()) >= 32
    assert sum(c["info"]["end"] == "sweep N" and c["info"]["sweeps"] == 1 for c in oc.values()) >= 32
    assert sum(c["info"]["end"].startswith("phase 2") for c in oc.values()) >= 64
    for n_ini in (1, 2, 3):
        assert sum(c["info"]["n_ini"] == n_ini for c in oc.values()) >= 32, n_ini
    strips = [c for c in oc.values() if c["args"][2] - c["args"][1] < c["args"][4] - c["args"][3]]
    assert len(strips) >= 32 and all(c["info"]["n_ini"] == 1 for c in strips)


def check_octree(res, mut=()):
    got = RC.unpack(res, "oct")
    assert len(got) == len(RC.octree_cases())
    for (name, c), g in zip(RC.octree_cases().items(), got):
        want = c["model"] if not mut else M.distribute(*c["args"], mut=mut)
        assert rows(g) == want, (name, c["info"])


@pytest.mark.parametrize("which", SOURCES)
def test_octree_tie_free(which):
    """the reference's vResultKeys == the model's in order, coordinates and response, on every kept seed"""
    check_octree(source(which))


# ---- the octree's hand-built cases ------------------------------------------------------------------------------------------------------------
def check_hand_octree(res, mut=(), live=None):
    """every DETECT case that reaches DistributeOctTree.  No tie: the reference == the model == the declared key-points, in order.  A
    tie: every order of every equal-size group is enumerated (the cap is not hit); the declared answer is one of the answers, and so is
    the live reference's (a tied case is never recorded)"""
    got = dict(zip(res["hand_names"].tolist(), RC.unpack(res, "hand")))
    tied = 0
    for name, c in RC.hand_octree().items():
        model = c["model"] if not mut else M.distribute(*c["args"], mut=mut)
        if not c["info"]["tie"]:
            assert rows(got[name]) == model == c["declared"], (name, rows(got[name]), model, c["declared"])
            continue
        tied += 1
        answers, hit = RC.enumerate_orders(c["args"])
        assert not hit and len(answers) >= 2 and c["declared"] in answers and c["model"] in answers, (name, answers)
        if live is not None:
            assert live.distribute(*c["args"]) in answers, name
    assert tied >= 1 and len(got) >= 30
    for must in ("float node edge below the rational@0", "phase 2, N passed by two@0", "a node one pixel wide@0", "an empty level@0"):
        assert must in got, must


def test_hand_built_octree_cases_recorded():
    check_hand_octree(RC.recorded())


def test_hand_built_octree_cases_live():
    check_hand_octree(source("live"), live=library())


# ---- the octree with ties, at scale -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_levels(seed):
    return M.pyramid(dev.scene(seed, (256, 224)), 8)


def test_octree_with_ties_at_scale_live():
    """dense 256 x 224 scenes, 8 levels, nfeatures 400 and 1 000: every level has a tie, so NOTHING is said about order.  Every result
    is one of the candidates; no candidate comes out twice (a node yields one key, and the nodes share none); the count is within
    level_bound; the count is at least min(N, the list's size when phase 1 ended) - phase 1 is tie-free and the list never shrinks.
    How often the declared order gave this host's answer is printed (DESIGN section 2 states one measurement), never asserted."""
    ref = library()
    equal = levels_seen = tied = 0
    for seed in (40, 41):
        for nfeatures in (400, 1000):
            per = M.features_per_level(nfeatures, 8)
            for l, img in enumerate(dense_levels(seed)):
                h, w = img.shape
                keys = [(x - B, y - B, s) for x, y, s in M.candidates(img)[0]]
                args, info = (keys, B, w - B, B, h - B, per[l]), {}
                model = M.distribute(*args, info=info)
                got = ref.distribute(*args)
                levels_seen += 1
                tied += info["tie"]
                equal += got == model
                assert info["tie"] or got == model, (seed, nfeatures, l)
                assert set(got) <= set(keys) and len(set(got)) == len(got), (seed, nfeatures, l)
                assert min(per[l], info["phase1"]) <= len(got) <= M.level_bound(w, h, per[l]), (seed, nfeatures, l, len(got))
    assert tied >= levels_seen * 3 // 4, (tied, levels_seen)
    print("ties at scale: %d of %d levels tied; the declared order gave this host's answer on %d" % (tied, levels_seen, equal))


# ---- the cell loop ----------------------------------------------------------------------------------------------------------------------------
def test_the_cell_scenes_are_what_they_are_for():
    sc = RC.cell_scenes()
    assert {"256x224", "92x92", "752x480"} <= set(sc) and sc["752x480"][0][0].shape == (480, 752)
    n_cols, n_rows, grid = M.cells(813, 92)
    assert len({j for _, j, *_ in grid}) == n_cols - 1  # :775 skipped the last column
    n_cols, n_rows, grid = M.cells(470, 903)
    assert len({i for i, *_ in grid}) == n_rows - 1  # :767 skipped the last row
    for name, (levels, nfeatures, ini_th, min_th) in sc.items():  # the single levels are tie-free, two of them through phase 2
        if len(levels) == 1 and not name.startswith("case/"):
            assert not M.detect(levels, nfeatures, 1.2, ini_th, min_th)["tie"][0], name
    assert M.detect(*sc["256x224"][:2])["sorts"][0] >= 1 and M.detect(*sc["last row skipped 470x903"][:2])["sorts"][0] >= 1
    for name in ("pyramid a", "pyramid b"):  # sparse enough: at least half of the levels that reach phase 2 are tie-free
        levels, nfeatures, ini_th, min_th = sc[name]
        m = M.detect(levels, nfeatures, 1.2, ini_th, min_th)
        reach = [l for l in range(8) if m["sorts"][l]]
        assert len(reach) >= 3 and 2 * sum(not m["tie"][l] for l in reach) >= len(reach), (name, m["sorts"], m["tie"])


@pytest.mark.parametrize("which", SOURCES)
def test_cell_grid(which):
    """a FAST that finds nothing: the record equals cells() in rectangles and order, every cell at 20 and again at 7; a level under 62 px
    (deviation 1) makes no call"""
    res = source(which)
    for name, calls in zip(res["cell_names"].tolist(), RC.unpack(res, "cell_empty_calls")):
        levels = RC.cell_scenes()[name][0]
        assert same(calls, RC.expected_calls(levels, lambda l, k: True)), name
    assert sum(res["cell_empty_calls_n"].tolist()) > 2 * (24 * 14 + 25 * 2 + 14 * 28)  # 752 x 480, 813 x 92 and 470 x 903 alone


def test_levels_without_a_cell_row_or_column_live():
    """deviation 1 as the reference has it under this compiler: its divisions by nCols / nRows = 0 are float divisions and trap nothing,
    no FAST call is made and no key-point comes back (the header states this outcome).  nIni is 0 on two of these levels as well:
    DistributeOctTree without a key returns nothing (deviation 2's harmless half)"""
    ref = library()
    for w, h in ((61, 92), (92, 61), (61, 61)):
        ref.set_hooks(fast=RC.model_fast)
        ref.set_levels([HC.flat(w, h, [(30, 30, 130)])], [50])
        ref.fast_calls()
        count, kp = ref.key_points()
        assert len(ref.fast_calls()) == 0 and len(kp) == 0 and not count.any() and not M.cells(w, h)[2], (w, h)
    assert ref.distribute([], 16, 46, 16, 116, 5) == []  # nIni = round(30 / 100) = 0


@pytest.mark.parametrize("which", SOURCES)
def test_scripted_key_points(which):
    """scripted answers: a cell that answered at 20 is not called again, every other cell is, and no call is made besides.  The scripted
    key-points - a cell's first and last computed pixel among them - come out shifted by (j wCell, i hCell) as candidates() says: with
    a count that :649's `size >= N` never reaches most come out (in the octree's order, the model's); with N = 1 each node of the first sweep
    gives the first of its equal responses, which shows the order in which the keys arrived.  The angle is ic_angle's."""
    res = source(which)
    total = 0
    for i, name in enumerate(res["cell_names"].tolist()):
        levels = RC.cell_scenes()[name][0]
        sc = RC.script(levels)
        want_calls = RC.expected_calls(levels, lambda l, k: sc.get((l, k), (0,))[0] != 20)
        for key, n in (("cell_all", RC.SCRIPT_ALL), ("cell_one", 1)):
            assert same(RC.unpack(res, key + "_calls")[i], want_calls), (name, key)
            model, tie = RC.scripted_model(levels, [n] * len(levels))
            want = RC.tie_free_rows(model, tie)
            got = RC.unpack(res, key + "_kp")[i]
            assert same(got[:, :5], want), (name, key)
            angle = np.array([orb_ref.ic_angle(levels[int(l)], int(x), int(y))[2] for x, y, l in got[:, :3]], np.float32)
            assert same(got[:, 5], angle), (name, key)
            if n == RC.SCRIPT_ALL:
                # (not every key need come out: a sweep whose divisions each keep their keys in one child ends the octree, :649)
                assert not any(tie) and 2 * len(got) >= sum(len(k) for k in RC.scripted_candidates(levels)), name
            total += len(got)
    assert total > 1000


def check_cell_fast(res, mut=()):
    at = 0
    fast_kp, fast_calls = RC.unpack(res, "cell_fast_kp"), RC.unpack(res, "cell_fast_calls")
    for name in res["cell_names"].tolist():
        levels, nfeatures, ini_th, min_th = RC.cell_scenes()[name]
        kp, m = RC.model_key_points(levels, nfeatures, ini_th, min_th, mut)
        assert same(fast_calls[at], RC.expected_calls(levels, RC.model_redo(levels, ini_th, mut), ini_th, min_th)), name
        assert same(fast_kp[at], RC.tie_free_rows(kp, m["tie"])), name
        at += 1
    assert at == len(fast_kp)


@pytest.mark.parametrize("which", SOURCES)
def test_cell_loop_with_the_models_fast(which):
    """cv::FAST answered by the model's fast_cell on the cell image the reference passed: cells that came back empty at ini_th are called
    again at min_th and no others; on every level the model calls tie-free, allKeypoints == detect()'s kp_xy, kp_oct, kp_response in
    order, size = (int)(31 mvScaleFactor[level]), angle == ic_angle's.  The sparse scenes, two eight-level pyramids, and every hand-built
    case with cells"""
    check_cell_fast(source(which))


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SOURCES)
def test_pyramid_sizes_and_views(which):
    """ComputePyramid: level sizes == level_sizes for every pair - sizes on or next to a half among them; each level is a view at (19, 19)
    of a matrix of (rows + 38) x (cols + 38), step cols + 38"""
    special, pairs = RC.pyramid_sizes()
    assert len(pairs) >= 20 and len(special) >= 16
    got = RC.unpack(source(which), "pyr")
    assert len(got) == len(pairs)
    for (w, h), g in zip(pairs, got):
        assert [tuple(r[:2]) for r in g.tolist()] == M.level_sizes(w, h, 8), (w, h)
        for rows_, cols, step, offset, store in g.tolist():
            assert (step, offset, store) == (cols + 38, 19 * (cols + 38) + 19, (rows_ + 38) * (cols + 38)), (w, h)


@pytest.mark.parametrize("which", SOURCES)
def test_pyramid_pixels(which):
    """with cv::resize answered by the model's resize, every level's pixels are the model's pyramid's"""
    got = RC.unpack(source(which), "pyr_px")
    at = 0
    for w, h in RC.PYRAMID_PIXELS:
        for want in M.pyramid(RC.pyramid_image(w, h), 8):
            assert same(got[at], want.reshape(-1)), (w, h)
            at += 1
    assert at == len(got)


def test_pyramid_hand_over_and_border_live():
    """each level is resized from the level BEFORE it (the source the reference passes is that level's view, bytes and shape); the
    matrix around a level is its BORDER_REFLECT_101 continuation (the stand-in's copyMakeBorder into a destination that already holds
    the level); and with every border byte overwritten ComputeKeyPointsOctTree gives the same answer: the border is never read - by the
    reference's own code; what OpenCV's FAST reads is not run here"""
    ref = library()
    for w, h in RC.PYRAMID_PIXELS:
        levels, seen = RC.live_pyramid(ref, RC.pyramid_image(w, h))
        assert len(levels) == 8 and len(seen) == 7
        for l, (src, shape) in enumerate(seen):
            assert same(src, levels[l]["pixels"]) and tuple(shape) == levels[l + 1]["shape"], (w, h, l)
        for lv in levels:
            assert same(lv["whole"].reshape(lv["shape"][0] + 38, lv["step"]), np.pad(lv["pixels"], 19, mode="reflect")), (w, h)
        ref.fast_calls()
        count, kp = ref.key_points()
        calls = ref.fast_calls()
        assert ref.overwrite_borders(5) == sum(lv["store"] - lv["shape"][0] * lv["shape"][1] for lv in levels)
        after = ref.levels()
        assert all(same(a["pixels"], b["pixels"]) and not same(a["whole"], b["whole"]) for a, b in zip(after, levels))
        count2, kp2 = ref.key_points()
        assert same(count, count2) and same(kp, kp2) and same(calls, ref.fast_calls()) and (len(kp) > 20 or w < 100), (w, h, len(kp))


# ---- the whole detect() -----------------------------------------------------------------------------------------------------------------------
def test_the_detect_scenes_are_what_they_are_for():
    for name in RC.DETECT_SCENES:
        m = RC.detect_model(name)[1]
        lc = m["level_count"]
        assert not any(m["tie"]) and sum(m["sorts"]) >= 2, (name, m["tie"], m["sorts"])
        assert any(lc[l] == 0 and lc[:l].sum() > 0 and lc[l + 1:].sum() > 0 for l in range(8)), (name, lc)


def check_detect(res, pattern=None):
    kps, descs, abs_ = (RC.unpack(res, k) for k in ("detect_kp", "detect_desc", "detect_ab"))
    for i, name in enumerate(RC.DETECT_SCENES):
        levels, m = RC.detect_model(name)
        kp, desc, ab = kps[i], descs[i], abs_[i]
        n = len(m["kp_oct"])
        assert len(kp) == len(desc) == len(ab) == n > 20, name
        assert same(kp[:, 2].astype(np.int32), m["kp_oct"]) and np.all(np.diff(kp[:, 2]) >= 0), name  # level-major, the empty level skipped
        blur_w = orb_ref.default_blur(2.0)
        flat = np.zeros((512, 2), np.int8) if pattern is None else pattern
        d = orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], flat, blur_w, ab=ab)  # the two models chained, steered by the reference host's (a, b)
        assert same(kp[:, :2], d["uv32"]), name  # pt after `*= mvScaleFactor[level]`, as float
        assert same(kp[:, 5], d["angle"]) and same(kp[:, 4], m["kp_response"]), name
        sf = orb_ref.scale_table(1.2)
        assert same(kp[:, 3], np.array([int(np.float32(31) * sf[l]) for l in m["kp_oct"]], np.float32)), name
        want_ab = np.array([orb_ref.steer(a) for a in kp[:, 5]], np.float32).reshape(-1, 2)
        assert np.all((ab == want_ab) | (ab == np.nextafter(want_ab, np.float32(np.inf))) | (ab == np.nextafter(want_ab, np.float32(-np.inf)))), name
        assert len(np.unique(desc, axis=0)) >= n // 2, name
        # computeDescriptors on the same key-points and angles under a pattern this project holds (what the device is held to)
        again = orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], orb_scenes.PATTERN, blur_w, ab=ab)
        assert same(RC.unpack(res, "detect_desc_pat")[i], again["desc"]), name
        if pattern is not None:
            assert same(desc, d["desc"]), (name, np.flatnonzero((desc != d["desc"]).any(axis=1)))


def test_detect_recorded():
    """_keypoints of the whole detect() against the two models chained - orb_detect_ref.detect, then orb_ref.describe: the order
    (level-major, the level without key-points skipped), pt * mvScaleFactor[level] as float, octave, size, response, angle.  The
    descriptors use the extractor's own pattern, which no file of this project holds: they are compared where the library is built"""
    check_detect(RC.recorded())


def test_detect_live():
    """as above, and _descriptors == orb_ref.describe with the extractor's own pattern, fetched from the library"""
    ref = library()
    pattern = ref.tables()["pattern"].astype(np.int8)
    check_detect(source("live"), pattern)
    check_detect(RC.recorded(), pattern)  # the recorded descriptors as well, each steered by its own host's (a, b)


# ---- every swapped rule is contradicted by the reference --------------------------------------------------------------------------------------
CONTRADICTED_BY = {"push_back": "N = 0@0", "floor_half": "floor for ceil@0", "rational_edge": "float node edge below the rational@0",
                   "level_fallback": "case/fallback per cell"}


@pytest.mark.parametrize("rule", sorted(CONTRADICTED_BY))
def test_the_reference_contradicts_each_swapped_rule(rule):
    """the model with one rule swapped differs from the RECORDED reference on the named hand-built case, and the pin test that holds that
    case fails.  `tie_rev` is the exception, below.  The rules of cv::FAST, cv::resize and cvRound (arc8, arc10, ge, score_off, nonstrict,
    nms_across, no_shift4, half_up) cannot be contradicted here: the stand-in answers them with the model itself"""
    res, name = RC.recorded(), CONTRADICTED_BY[rule]
    if rule == "level_fallback":
        levels, nfeatures, ini_th, min_th = RC.cell_scenes()[name]
        at = res["cell_names"].tolist().index(name)
        kp, m = RC.model_key_points(levels, nfeatures, ini_th, min_th, (rule,))
        assert not any(m["tie"]) and not same(RC.unpack(res, "cell_fast_kp")[at], kp)
        with pytest.raises(AssertionError):
            check_cell_fast(res, (rule,))
    else:
        c = RC.hand_octree()[name]
        got = dict(zip(res["hand_names"].tolist(), RC.unpack(res, "hand")))[name]
        assert not c["info"]["tie"] and rows(got) != M.distribute(*c["args"], mut=(rule,))
        with pytest.raises(AssertionError):
            check_hand_octree(res, (rule,))
    check_hand_octree(res)
    check_cell_fast(res)


def test_the_reference_cannot_contradict_the_declared_tie_order():
    """`tie_rev`: on the tied hand-built case the declared answer and the reversed one are both among the enumerated answers, and so is
    the live reference's whichever it is: where sizes tie the reference puts neither order in the wrong.  On every tie-free case tie_rev
    changes nothing"""
    c = RC.hand_octree()["two equal sizes in phase 2@0"]
    answers, hit = RC.enumerate_orders(c["args"])
    rev = M.distribute(*c["args"], mut=("tie_rev",))
    assert not hit and c["declared"] in answers and rev in answers and rev != c["declared"]
    assert sorted(map(tuple, RC.enumerate_orders(c["args"], mut=("tie_rev",))[0])) == sorted(map(tuple, answers))
    ref = oracle_lib.load_orb_ref()
    if ref is not None and ref._detect_half:
        assert ref.distribute(*c["args"]) in answers
    check_octree(RC.recorded(), ("tie_rev",))


def test_live_and_recorded_agree():
    """everything recorded is tie-free and holds no libm result but detect()'s (a, b) and the descriptors they steer"""
    live, rec = source("live"), RC.recorded()
    assert sorted(live) == sorted(rec)
    for k in rec:
        if k not in ("detect_ab", "detect_desc", "detect_desc_pat"):
            assert same(live[k], rec[k]), k
