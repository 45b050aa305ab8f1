"""CPU: the sequential model of gl_orb_pyramid / gl_orb_detect (tests/orb_detect_ref.py) gives every DECLARED output of
tests/orb_detect_cases.py; a second statement of FAST, the suppression and the resize - written another way - agrees with it on random
images; and every rule swapped on purpose is seen by at least one declared case."""
import numpy as np
import pytest

from tests import orb_detect_cases as cases
from tests import orb_detect_dev as dev
from tests import orb_detect_ref as ref


def as_call(m, cand_cap):
    """one image's model outputs in the call's layout"""
    N = max(len(m["kp_oct"]), 1) + 3
    return {k: v[0] for k, v in dev.expected([m], N, cand_cap).items()}


def run_case(name, mut=()):
    c = cases.DETECT[name]
    return as_call(ref.detect(c["levels"], c["nfeatures"], 1.2, c["ini_th"], c["min_th"], c["cand_cap"], mut), c["cand_cap"])


@pytest.mark.parametrize("name", sorted(cases.DETECT))
def test_model_gives_the_declared_outputs(name):
    cases.check_declared(name, run_case(name))


@pytest.mark.parametrize("name", sorted(cases.RESIZE))
def test_model_gives_the_declared_levels(name):
    c = cases.RESIZE[name]
    cases.check_declared_resize(name, ref.pyramid(c["image"], c["nlevels"], c["scale_factor"]))


# ---- a second statement
def score_by_trial(img, x, y):
    """the largest t >= 0 at which the segment test passes, found by trying every t; -1: none"""
    v = int(img[y, x])
    p = [int(img[y + dy, x + dx]) for dx, dy in ref.RING]
    best = -1
    for t in range(255):
        ok = any(all(p[(k + j) % 16] > v + t for j in range(9)) or all(p[(k + j) % 16] < v - t for j in range(9)) for k in range(16))
        if not ok:
            break
        best = t
    return best


@pytest.mark.parametrize("seed", [0, 1])
def test_fast_by_trial_agrees(seed):
    img = dev.scene(seed, (70, 66))
    x0, y0, x1, y1 = 16, 16, 54, 50  # one cell image
    for th in (7, 20):
        s = np.zeros((y1 - y0, x1 - x0), np.int64)
        for y in range(y0 + 3, y1 - 3):
            for x in range(x0 + 3, x1 - 3):
                t = score_by_trial(img, x, y)
                s[y - y0, x - x0] = t if t >= th else 0
        keys = []
        for y in range(3, y1 - y0 - 3):  # rows, then columns; everything outside the region is 0 already
            for x in range(3, x1 - x0 - 3):
                nb = s[y - 1:y + 2, x - 1:x + 2].copy()
                nb[1, 1] = -1
                if s[y, x] > 0 and s[y, x] > nb.max():
                    keys.append((x0 + x, y0 + y, int(s[y, x])))
        got = ref.fast_cell(img, x0, y0, x1, y1, th)
        assert len(got) > 3 and got == keys, th


def test_resize_in_rationals_agrees():
    """the coefficients from exact fractions where the float chain is exact (power-of-two ratios), the pixel from the declared shifts"""
    img = dev.scene(3, (64, 48))
    got = ref.resize(img, (24, 32))
    S = img.astype(np.int64)
    for dy in range(24):
        for dx in range(32):
            r = [1024 * S[2 * dy + j, 2 * dx] + 1024 * S[2 * dy + j, 2 * dx + 1] for j in (0, 1)]
            assert got[dy, dx] == (((1024 * (r[0] >> 4)) >> 16) + ((1024 * (r[1] >> 4)) >> 16) + 2) >> 2
    levels = ref.pyramid(dev.scene(4), 4)
    assert [l.shape for l in levels] == [(120, 160), (100, 133), (83, 111), (69, 93)]
    for a, b in zip(levels, levels[1:]):  # a bilinear mean stays within the source's range and near its mean
        assert b.min() >= a.min() and b.max() <= a.max() and abs(float(b.mean()) - float(a.mean())) < 2.0


def test_features_per_level_of_the_reference_defaults():
    assert ref.features_per_level(1000, 8) == [217, 181, 151, 126, 105, 87, 73, 60]
    assert sum(ref.features_per_level(2000, 8)) == 2000 and ref.features_per_level(0, 1) == [0]


# ---- every swapped rule is seen by a declared case
SEEN_BY = {"ge": "brighter by th", "arc8": "arc of 8", "arc10": "arc of 9", "score_off": "brighter by th + 1", "nonstrict": "equal adjacent scores",
           "nms_across": "adjacent across a cell boundary", "level_fallback": "fallback per cell", "push_back": "N = 0",
           "tie_rev": "two equal sizes in phase 2", "floor_half": "floor for ceil", "rational_edge": "float node edge below the rational"}
# (the resize's two swapped rules, "half_up" and "no_shift4", are seen in test_swapped_resize_rules_are_seen)


@pytest.mark.parametrize("mut", [m for m, n in SEEN_BY.items() if n and n in cases.DETECT])
def test_swapped_rule_is_seen(mut):
    with pytest.raises(AssertionError):
        cases.check_declared(SEEN_BY[mut], run_case(SEEN_BY[mut], (mut,)))


def test_swapped_resize_rules_are_seen():
    c = cases.RESIZE["sizes on a half"]
    with pytest.raises(AssertionError):  # half up: cvRound(2.5) = 3
        cases.check_declared_resize("sizes on a half", ref.pyramid(c["image"], c["nlevels"], c["scale_factor"], ("half_up",)))
    # half up against half to even in a coefficient: every column of this case has fx x 2048 on a half
    c = cases.RESIZE["coefficients on a half"]
    for mut in ("half_up", "no_shift4"):  # (the shift dropped: b (r >> 4) >> 16 against (b r) >> 20 differ where r's low four bits carry)
        with pytest.raises(AssertionError):
            cases.check_declared_resize("coefficients on a half", ref.pyramid(c["image"], c["nlevels"], c["scale_factor"], (mut,)))
    assert ref.cv_round(np.float32(0.5)) == 0 and ref.cv_round(np.float32(0.5), ("half_up",)) == 1
    assert ref.cv_round(np.float32(1.5)) == 2 and ref.cv_round(np.float32(2.5)) == 2
