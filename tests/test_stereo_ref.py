"""CPU: the sequential model of Frame::computeStereoMatches (tests/stereo_ref.py) gives every DECLARED output of tests/stereo_cases.py; a
second, vectorised statement of the function agrees with it on the random scenes; and every rule of the model, swapped for its
neighbour, changes at least one declared case - the cases can see each rule."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from tests import stereo_cases, stereo_ref, stereo_scenes

f32, f64 = np.float32, np.float64
KEYS = ("feat_ur", "feat_depth", "match_r", "sad", "stat")


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", sorted(stereo_cases.CASES))
def test_model_gives_the_declared_outputs(name):
    c = stereo_cases.CASES[name]
    got = stereo_ref.stereo_matches(stereo_cases.CAM, stereo_cases.SCALE, **c["frame"])
    for k in KEYS:
        assert bits_equal(got[k], c["expect"][k]), (name, k, got[k], c["expect"][k])


def test_cases_cover_the_issues_list():
    assert len(stereo_cases.CASES) >= 80
    for c in stereo_cases.CASES.values():
        assert all(im.shape[0] <= 48 and im.shape[1] <= 64 for im in c["frame"]["pyr_left"] + c["frame"]["pyr_right"])
        assert len(c["frame"]["feat_oct"]) <= 4 and len(c["frame"]["r_oct"]) <= 4


# ---- the second statement: whole arrays at a time, no row table, no running minimum
def round_away(x):
    return np.copysign(np.floor(np.abs(x) + x.dtype.type(0.5)), x)  # (|x| + 0.5 is exact below 2^22 for the halves met here)


def vectorised(cam, scale_factor, feat_uv, feat_oct, feat_desc, r_uv, r_oct, r_desc, pyr_left, pyr_right):
    fx, bf, H = cam
    nlev = len(pyr_left)
    sf, inv = stereo_ref.scale_tables(scale_factor)
    NF = len(feat_oct)
    mbf = f32(bf)
    maxD = f32(mbf / f32(f64(bf) / f64(fx)))
    okr = (r_oct >= 0) & (r_oct < nlev)
    r = (f32(2.0) * sf[np.clip(r_oct, 0, 7)]).astype(f32)
    maxr, minr = np.ceil((r_uv[:, 1] + r).astype(f32)), np.floor((r_uv[:, 1] - r).astype(f32))
    vL, uL = feat_uv[:, 1].astype(f32), feat_uv[:, 0].astype(f32)
    okl = (feat_oct >= 0) & (feat_oct < nlev) & (vL >= 0) & (vL < H) & ~(uL < 0)
    row = np.trunc(vL)
    cand = (okl[:, None] & okr[None, :] & (minr[None, :] <= row[:, None]) & (row[:, None] <= maxr[None, :]) &
            (np.abs(r_oct[None, :] - feat_oct[:, None]) <= 1) & (r_uv[None, :, 0] >= (uL - maxD).astype(f32)[:, None]) & (r_uv[None, :, 0] <= uL[:, None]))
    dist = np.unpackbits(feat_desc[:, None, :] ^ r_desc[None, :, :], axis=2).sum(axis=2).astype(np.int64)
    key = np.where(cand & (dist < 100), dist * 4096 + np.arange(len(r_oct))[None, :], 100 * 4096)
    best = key.min(axis=1)
    passed = best // 4096 < 75
    out = dict(feat_ur=np.full(NF, -1.0, f32), feat_depth=np.full(NF, -1.0, f32), match_r=np.full(NF, -1, np.int32), sad=np.full(NF, -1, np.int32))
    for i in np.flatnonzero(passed):
        l, iR = int(feat_oct[i]), int(best[i] % 4096)
        cu, cv = (round_away(feat_uv[i] * f64(inv[l]))).astype(f32)
        cr = round_away(np.array(f32(r_uv[iR, 0] * inv[l])))
        IL, IR = pyr_left[l].astype(np.int64), pyr_right[l].astype(np.int64)
        if not (cr >= 10 and cr + 11 < IR.shape[1] and cu >= 5 and cu + 5 < IL.shape[1] and cv >= 5 and cv + 5 < min(IL.shape[0], IR.shape[0])):
            continue
        cu, cv, cr = int(cu), int(cv), int(cr)
        wl = IL[cv - 5:cv + 6, cu - 5:cu + 6] - IL[cv, cu]
        strip = IR[cv - 5:cv + 6, cr - 10:cr + 11]
        wins = sliding_window_view(strip, 11, axis=1) - strip[5, 5:16][None, :, None]   # (11 rows, 11 incR, 11 columns)
        sads = np.abs(wins - wl[:, None, :]).sum(axis=(0, 2))
        k = int(np.argmin(sads))  # the first of the minima
        if k in (0, 10):
            continue
        d1, d2, d3 = (f32(sads[k - 1]), f32(sads[k]), f32(sads[k + 1]))
        delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if delta < -1 or delta > 1:
            continue
        bu = f32(sf[l] * f32(f32(f32(cr) + f32(k - 5)) + delta))
        disp = f32(uL[i] - bu)
        if not (disp >= 0 and disp < maxD):
            continue
        if disp <= 0:
            disp, bu = f32(0.01), f32(f64(uL[i]) - f64(0.01))
        out["feat_ur"][i], out["feat_depth"][i], out["match_r"][i], out["sad"][i] = bu, f32(mbf / disp), iR, sads[k]
    lst = np.sort(out["sad"][out["sad"] >= 0])
    median, nreset = -1, 0
    if len(lst):
        median = int(lst[len(lst) // 2])
        gone = (out["sad"] >= 0) & (out["sad"].astype(f32) >= f32(f32(f32(1.5) * f32(1.4)) * f32(median)))
        out["feat_ur"][gone] = out["feat_depth"][gone] = -1.0
        nreset = int(gone.sum())
    out["stat"] = np.array([passed.sum(), len(lst), nreset, median], np.int32)
    return out


SCENES = {("random", s): dict(seed=s) for s in range(4)}
SCENES.update({("levels", 8): dict(seed=308, size=(320, 240), nlevels=8, nfeat=200), ("levels", 1): dict(seed=301, size=(320, 240), nlevels=1, nfeat=200),
               "band300": dict(seed=77, nlevels=1, nfeat=300, row=60)})


@pytest.mark.parametrize("key", list(SCENES), ids=str)
def test_vectorised_statement_agrees(key):
    scene = stereo_scenes.random_scene(**SCENES[key])
    m = stereo_scenes.model_of(key, scene)
    v = vectorised(scene["cam"], scene["scale_factor"], **scene["frame"])
    for k in KEYS:
        assert bits_equal(v[k], m[k]), (key, k)


@pytest.mark.parametrize("seed", range(4))
def test_random_scenes_exercise_the_rules(seed):
    """what tests/test_gpu_stereo.py asks of a scene before it runs it on the device"""
    m = stereo_scenes.model_of(("random", seed), stereo_scenes.random_scene(seed))
    assert (m["feat_depth"] > 0).sum() >= 0.4 * len(m["sad"]) and m["stat"][2] >= 1
    assert all(m["dropped"][line] >= 1 for line in (261, 306, 325)), m["dropped"]


# A rule whose neighbour gives the same bits on EVERY input cannot be seen by any case; each with the reason:
UNOBSERVABLE = {
    "init_le": "a distance of 100 that updates the best still fails `bestDist < 75` (:261)",
    "delta_double": "a float quotient through double is the correctly rounded float quotient (53 >= 2 x 24 + 2 bits)",
    "zero_branch_float": "(float)(uL - 0.01f) == (float)((double)uL - 0.01) wherever bestuR == uL can happen on these level grids (searched)",
    "th_double": "for no median up to 61 710 (the largest SAD) does an integer lie between 2.0999999f x median and 2.0999999999999996 x median (searched)",
}


@pytest.mark.parametrize("rule", stereo_ref.MUTATIONS)
def test_each_rule_is_seen_by_a_case(rule):
    changed = []
    for name, c in stereo_cases.CASES.items():
        got = stereo_ref.stereo_matches(stereo_cases.CAM, stereo_cases.SCALE, mut=(rule,), **c["frame"])
        if any(not bits_equal(got[k], c["expect"][k]) for k in KEYS):
            changed.append(name)
    if rule in UNOBSERVABLE:
        assert not changed, "%s is listed as unobservable (%s) but changes %s" % (rule, UNOBSERVABLE[rule], changed)
    else:
        assert changed, "no declared case sees the rule %s" % rule
