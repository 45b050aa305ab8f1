"""gl_orb_pyramid, gl_orb_detect and orb.extract on the device against the reference's OWN ORB extractor: what oracle/_ref/liborb_ref.so
gave for the cases of tests/orb_detect_ref_cases.py, as recorded in tests/golden/golden_orb_detect_ref.npz (the reference tree itself is never
read here), and the live library as well where it has been built.  Bit for bit, on every level whose octree the model calls tie-free; where
a phase-2 sort sees equal sizes the reference's answer is its allocator's (deviation 4 of gl_orb_detect) and nothing is compared.

Of the octree cases only those BUILT FROM IMAGES can go through gl_orb_detect: the hand-built cases of tests/orb_detect_cases.py (isolated
dots) and the cell-loop scenes.  The seeded key sets of the CPU pin are arbitrary points in arbitrary order, which no image hands to the
octree; they stay with the model (tests/test_orb_detect_ref_pin.py), and the model with the device (tests/test_gpu_orb_detect.py).
cv::FAST, cv::resize and cvRound are the model's in the recording too: this module pins the device to the reference's code AROUND them."""
import numpy as np
import pytest

from tests import oracle_lib, orb_ref, orb_scenes
from tests import orb_detect_cases as HC
from tests import orb_detect_dev as dev
from tests import orb_detect_ref as M
from tests import orb_detect_ref_cases as RC
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu
B = M.MIN_BORDER
CAP = 2048


@pytest.fixture(scope="module")
def sources():
    """[(label, {key: array})]: the recorded file, and the live library's answers where oracle/_ref/liborb_ref.so is present"""
    ref = oracle_lib.load_orb_ref()
    return [("recorded", RC.recorded())] + ([("live", RC.live(ref))] if ref is not None and ref._detect_half else [])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the tie-free octree cases that were built from images -------------------------------------------------------------------------------------
def hand_cases():
    """the DETECT cases of which every level that reaches DistributeOctTree is tie-free (and at least one does), by group"""
    per_case = {}
    for key, c in RC.hand_octree().items():
        per_case.setdefault(key.rsplit("@", 1)[0], []).append(c["info"]["tie"])
    groups = {}
    for name, ties in per_case.items():
        c = HC.DETECT[name]
        if not any(ties) and c["mask"] == 0:  # one call: one geometry and one set of parameters
            groups.setdefault((c["group"], c["nfeatures"], c["N"], c["ini_th"], c["min_th"], c["cand_cap"]), []).append(name)
    return groups


def reference_key_points(res, name):
    """the recorded vResultKeys of every level of a hand-built case, in the call's coordinates -> (kp_xy, kp_oct, kp_response)"""
    got = dict(zip(res["hand_names"].tolist(), RC.unpack(res, "hand")))
    xy, octs, resp = [], [], []
    for l in range(len(HC.DETECT[name]["levels"])):
        for x, y, r in got.get("%s@%d" % (name, l), np.zeros((0, 3), np.int32)).tolist():
            xy.append((x + B, y + B))
            octs.append(l)
            resp.append(r)
    return np.array(xy, np.int32).reshape(-1, 2), np.array(octs, np.int32), np.array(resp, np.float32)


def check_hand(gpu, sources, names, label):
    torch, ctx = gpu
    c = HC.DETECT[names[0]]
    frames = [HC.DETECT[n]["levels"] for n in names]
    N = c["N"] or max(sum(M.level_bound(l.shape[1], l.shape[0], n) for l, n in zip(f, M.features_per_level(c["nfeatures"], len(f)))) for f in frames)
    got = dev.run(torch, ctx, frames, c["nfeatures"], max(N, 1), c["cand_cap"], ini_th=c["ini_th"], min_th=c["min_th"])
    for what, res in sources:
        for b, name in enumerate(names):
            xy, octs, resp = reference_key_points(res, name)
            n = len(octs)
            assert n >= 1 and int(got["n_kp"][b]) == n, (label, what, name, int(got["n_kp"][b]), n)
            assert same(got["kp_xy"][b, :n], xy) and same(got["kp_oct"][b, :n], octs) and same(got["kp_response"][b, :n], resp), (label, what, name)


def test_hand_built_cases_alone(gpu, sources):
    """B = 1: every hand-built case whose octree is tie-free == the reference's DistributeOctTree on that case's candidates, in order"""
    groups = hand_cases()
    assert sum(len(v) for v in groups.values()) >= 30
    for names in groups.values():
        for name in names:
            check_hand(gpu, sources, [name], name)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_hand_built_cases_as_one_batch(gpu, sources, order):
    """every group (one geometry and one set of parameters) as ONE call, in both orders"""
    for group, names in sorted(hand_cases().items(), key=lambda kv: str(kv[0])):
        check_hand(gpu, sources, sorted(names, reverse=order == "descending"), "group %s %s" % (group, order))


# ---- the cell-loop scenes and the two whole-detect() scenes through orb.extract ----------------------------------------------------------------
def extract(gpu, images, nfeatures, nlevels):
    from gmmloc_amd import orb
    torch, ctx = gpu
    d = torch.device("cuda:0")
    pyr, det, des = orb.extract(ctx, torch.from_numpy(np.stack(images)).to(d), torch.from_numpy(orb_scenes.PATTERN).to(d), nfeatures=nfeatures,
                                nlevels=nlevels, cand_cap=CAP)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in det.items()}
    out.update({k: v.cpu().numpy() for k, v in des.items()})
    return out


CELL_IMAGES = {"256x224": (lambda: RC.sparse(1, (256, 224), 120), 1), "256x224, count never reached": (lambda: RC.sparse(1, (256, 224), 120), 1),
               "92x92": (lambda: RC.sparse(2, (92, 92), 14), 1),
               "pyramid a": (lambda: RC.sparse(6, (256, 224), 150), 8), "pyramid b": (lambda: RC.sparse(7, (256, 224), 220), 8)}


@pytest.mark.parametrize("name", sorted(CELL_IMAGES))
def test_cell_loop_scene_through_extract(gpu, sources, name):
    """orb.extract on the raw image: on every tie-free level the key-points, responses, angles and uv32 are the reference's allKeypoints
    (ComputeKeyPointsOctTree with its FAST answered by the model's), in order"""
    make, nlevels = CELL_IMAGES[name]
    levels, nfeatures, _, _ = RC.cell_scenes()[name]
    image = make()
    assert len(levels) == nlevels and same(image, levels[0])
    got = extract(gpu, [image], nfeatures, nlevels)
    tie = M.detect(levels, nfeatures)["tie"]
    n = int(got["n_kp"][0])
    keep = np.array([not tie[l] for l in got["kp_oct"][0, :n]], bool).reshape(-1)
    sf = orb_ref.scale_table(1.2)
    for what, res in sources:
        kp = RC.unpack(res, "cell_fast_kp")[res["cell_names"].tolist().index(name)]
        assert len(kp) >= 8 and int(keep.sum()) == len(kp), (name, what, int(keep.sum()), len(kp))
        assert same(got["kp_xy"][0, :n][keep].astype(np.float32), kp[:, :2]) and same(got["kp_oct"][0, :n][keep].astype(np.float32), kp[:, 2]), (name, what)
        assert same(got["kp_response"][0, :n][keep], kp[:, 4]) and same(got["angle"][0, :n][keep], kp[:, 5]), (name, what)
        scale = np.array([sf[int(l)] if l else np.float32(1) for l in kp[:, 2]], np.float32)
        assert same(got["uv32"][0, :n][keep], kp[:, :2] * scale[:, None]), (name, what)


def test_whole_detect_scenes_through_extract(gpu, sources):
    """the two scenes of the whole detect() as one batch, in both orders: n_kp, octaves (level-major, the level without key-points
    skipped), uv32 = pt after `*= scale`, angles and responses are detect()'s _keypoints bit for bit.  Descriptors: the reference's
    computeDescriptors on those key-points under orb_scenes.PATTERN (detect() itself uses the extractor's own pattern, which this project
    does not hold) wherever the recording host's (a, b) is the declared steering; elsewhere the model's under the declared steering"""
    names = list(RC.DETECT_SCENES)
    for order in (names, names[::-1]):
        nf = {RC.detect_scene(n)[1] for n in order}
        runs = [extract(gpu, [RC.detect_scene(n)[0] for n in order], f, 8) for f in sorted(nf)]  # (one call per nfeatures)
        for what, res in sources:
            for b, name in enumerate(order):
                i = names.index(name)
                got = runs[sorted(nf).index(RC.detect_scene(name)[1])]
                kp, ab, desc = (RC.unpack(res, k)[i] for k in ("detect_kp", "detect_ab", "detect_desc_pat"))
                n = len(kp)
                assert int(got["n_kp"][b]) == n and same(got["kp_oct"][b, :n].astype(np.float32), kp[:, 2]), (name, what)
                assert same(got["uv32"][b, :n], kp[:, :2]) and same(got["angle"][b, :n], kp[:, 5]) and same(got["kp_response"][b, :n], kp[:, 4]), (name, what)
                declared = np.array([orb_ref.steer(a) for a in kp[:, 5]], np.float32).reshape(-1, 2)
                by_ref = (declared.view(np.uint32) == np.ascontiguousarray(ab).view(np.uint32)).all(axis=1)
                levels, m = RC.detect_model(name)
                model = orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], orb_scenes.PATTERN, orb_ref.default_blur(2.0))["desc"]
                want = np.where(by_ref[:, None], desc, model)
                print("%s (%s): %d of %d descriptors held to the model, not the reference (libm's steering is not the declared one)" %
                      (name, what, int((~by_ref).sum()), n))
                assert same(got["desc"][b, :n], want), (name, what, np.flatnonzero((got["desc"][b, :n] != want).any(axis=1)))
                assert not got["desc"][b, n:].any() and np.all(got["kp_oct"][b, n:] == -1), (name, what)


# ---- the cell grid at 752 x 480 ----------------------------------------------------------------------------------------------------------------
def test_candidates_752x480_follow_the_recorded_cells(gpu, sources):
    """cand_count and the candidate list of one 752 x 480 level == the model's FAST run over the rectangles that the REFERENCE passed to
    cv::FAST, in its order, each at the threshold of that cell's last call; the key-points == the reference's allKeypoints (a count
    that is never reached: every sweep of phase 1 runs and phase 2 never starts, so no tie can arise)"""
    torch, ctx = gpu
    levels, nfeatures, ini_th, min_th = RC.cell_scenes()["752x480"]
    img = levels[0]
    got = dev.run(torch, ctx, [levels], nfeatures, M.level_bound(752, 480, nfeatures), CAP)
    assert not M.detect(levels, nfeatures)["tie"][0]
    for what, res in sources:
        calls = RC.unpack(res, "cell_fast_calls")[res["cell_names"].tolist().index("752x480")]
        last = {}
        for _, x0, y0, cols, rows, th, _ in calls.tolist():  # (a cell called twice keeps its second threshold; dicts keep the first order)
            last[(x0, y0, cols, rows)] = th
        assert len(last) == 24 * 14 and len(calls) > len(last)  # width 720 / 30 = 24 columns, height 448 / 30 = 14.9: 14 rows
        cand = [k for (x0, y0, cols, rows), th in last.items() for k in M.fast_cell(img, x0, y0, x0 + cols, y0 + rows, th)]
        n = len(cand)
        assert n > 300 and got["cand_count"][0].tolist() == [n] + [0] * 7, (what, n, got["cand_count"][0])
        ca = np.array(cand, np.int64)
        assert np.array_equal(got["cand_xy"][0, 0, :n], ca[:, :2]) and np.array_equal(got["cand_resp"][0, 0, :n], ca[:, 2].astype(np.float32)), what
        assert int(got["stat"][0, 1]) == len(calls) - len(last), what
        kp = RC.unpack(res, "cell_fast_kp")[res["cell_names"].tolist().index("752x480")]  # tie-free: the count is never reached
        m = len(kp)
        assert m > 300 and int(got["n_kp"][0]) == m and same(got["kp_xy"][0, :m].astype(np.float32), kp[:, :2]), what
        assert same(got["kp_response"][0, :m], kp[:, 4]), what


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------------------
def test_pyramid_sizes_and_hand_over(gpu, sources):
    """gl_orb_pyramid_layout's level sizes == ComputePyramid's for every recorded pair (sizes on or next to a half among them); the
    device's levels == the reference's pyramid's pixels (each level resized from the one before it by the model's resize)"""
    from gmmloc_amd import orb
    torch, ctx = gpu
    pairs = RC.pyramid_sizes()[1]
    for what, res in sources:
        for (w, h), g in zip(pairs, RC.unpack(res, "pyr")):
            c = orb.pyramid_layout(w, h, 8)
            assert [[c.height[l], c.width[l]] for l in range(8)] == g[:, :2].tolist(), (what, w, h)
        px = RC.unpack(res, "pyr_px")
        at = 0
        for w, h in RC.PYRAMID_PIXELS:
            frames = dev.run_pyramid(torch, ctx, [RC.pyramid_image(w, h)], 8, row_pad=3, lead=5)
            for l in range(8):
                assert same(frames[0][l].reshape(-1), px[at]), (what, w, h, l)
                at += 1
