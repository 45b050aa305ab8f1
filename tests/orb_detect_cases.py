"""Hand-built cases of gl_orb_pyramid and gl_orb_detect, each with DECLARED outputs: the numbers below are worked out by hand from the
rules in include/gmmloc_hip.h, not produced by the model or the device.  tests/test_orb_detect_ref.py holds the model to them,
tests/test_gpu_orb_detect.py the device.  One case on each side of a decision.

The images are flat (100) with single pixels set.  A lone pixel of value v is a corner with all sixteen differences v - 100, so its
score is |v - 100| - 1; pixels that only lower a difference of the centre's ring stay within the threshold of the background, so they
are no corners themselves.  Unless a case says otherwise the level is 92 x 92: borders 16 and 76, width = 60, nCols = nRows = 2, wCell =
hCell = 30; cell column 0 computes x in [19, 49), column 1 x in [49, 73); nIni = 1, the root node is [0, 60) x [0, 60) in the octree's
coordinates (x - 16, y - 16) and its halves meet at 30.

Not reachable through the entry point, hence without a case: the resize's clamp at sx < 0 (it needs an enlarging step; a pyramid only
shrinks).  Two keys that fall into one child leave the list's size as it was, which ends the octree (:649); a node one pixel wide
needs further keys that keep the list growing.  Test infrastructure; nothing in the product imports it."""
import numpy as np

from tests.orb_detect_ref import RING

BG = 100


def flat(w=92, h=92, dots=()):
    img = np.full((h, w), BG, np.uint8)
    for x, y, v in dots:
        img[y, x] = v
    return img


def ring(x, y, values):
    """pixels on the ring of (x, y): {ring position: value}"""
    return [(x + RING[k][0], y + RING[k][1], v) for k, v in values.items()]


def rel(*pts):
    """dots of value 130 at octree coordinates"""
    return [(x + 16, y + 16, v[0] if v else 130) for x, y, *v in pts]


def case(group, dots, kp, cand=None, fell=None, nfeatures=50, size=(92, 92), th=(20, 20), cand_cap=64, mask=0, levels=None, N=None):
    """kp: the declared key-points [(x, y, octave, response)] in order; cand: the declared candidates of level 0 [(x, y, score)] (None:
    the key-points' own, which holds when every candidate survives in candidate order); fell: the declared count of cells redone"""
    levels = [flat(size[0], size[1], dots)] if levels is None else levels
    return dict(group=group, levels=levels, nfeatures=nfeatures, ini_th=th[0], min_th=th[1], cand_cap=cand_cap, kp=kp, cand=cand, fell=fell, mask=mask,
                N=N)


C = (40, 40)  # a pixel of cell (0, 0)
DETECT = {
    # ---- the segment test (ini_th = min_th = 20: a redone cell finds what it found)
    "arc of 9": case("fast", [(40, 40, 130)] + ring(40, 40, {k: 112 for k in range(7)}), [(40, 40, 0, 29)], fell=3),
    "arc of 8": case("fast", [(40, 40, 130)] + ring(40, 40, {k: 112 for k in range(8)}), [], fell=4),
    "brighter by th": case("fast", [(40, 40, 120)], [], fell=4),
    "brighter by th + 1": case("fast", [(40, 40, 121)], [(40, 40, 0, 20)], fell=3),
    "darker by th": case("fast", [(40, 40, 80)], [], fell=4),
    "darker by th + 1": case("fast", [(40, 40, 79)], [(40, 40, 0, 20)], fell=3),
    # every arc of 9 holds ring position 0 (difference 40) or 8 (difference 45): the arcs without position 0 give 45, the others 40
    "two competing arcs": case("fast", [(40, 40, 160)] + ring(40, 40, {0: 120, 8: 115}), [(40, 40, 0, 44)], fell=3),
    # ---- suppression and cells
    "equal adjacent scores": case("fast", [(40, 40, 130), (41, 40, 130)], [], fell=4),
    "unequal adjacent scores": case("fast", [(40, 40, 130), (41, 40, 131)], [(41, 40, 0, 30)], fell=3),
    # 48 | 49 is the cells' boundary: both stay; the root's only child [30, 60) x [0, 30) holds both, the list does not grow (:649) and
    # the first of equals is picked
    "adjacent across a cell boundary": case("fast", [(48, 40, 130), (49, 40, 130)], [(48, 40, 0, 29)], cand=[(48, 40, 29), (49, 40, 29)], fell=2),
    "first computed pixel of the level": case("fast", [(19, 19, 130)], [(19, 19, 0, 29)], fell=3),
    "one before the first computed column": case("fast", [(18, 40, 130)], [], fell=4),
    "last computed pixel of the level": case("fast", [(72, 72, 130)], [(72, 72, 0, 29)], fell=3),
    "one behind the last computed row": case("fast", [(40, 73, 130)], [], fell=4),
    # (48, 48) closes cell (0, 0), (49, 20) opens cell (0, 1); they fall into n4 and n2, and n4 was pushed last
    "last pixel of a cell, first of the next": case("fast", [(48, 48, 130), (49, 20, 131)], [(48, 48, 0, 29), (49, 20, 0, 30)],
                                                    cand=[(48, 48, 29), (49, 20, 30)], fell=2),
    # ---- thresholds 20 / 7: cell (0, 0) holds a weak corner alone and is redone; cell (0, 1) holds a strong one, so its weak one is absent.
    # The root's children: n2 (the strong one) was pushed last and stands first
    "fallback per cell": case("threshold", [(30, 30, 110), (60, 30, 130), (65, 40, 110)], [(60, 30, 0, 29), (30, 30, 0, 9)],
                              cand=[(30, 30, 9), (60, 30, 29)], fell=3, th=(20, 7)),
    "contrast of min_th": case("threshold", [(30, 30, 107)], [], fell=4, th=(20, 7)),
    "contrast of min_th + 1": case("threshold", [(30, 30, 108)], [(30, 30, 0, 7)], fell=4, th=(20, 7)),
    # ---- cell geometry
    "width 61: no cell column": case("w61", [(30, 40, 130)], [], fell=0, size=(61, 92)),
    # width = 30: one column, x in [19, 43); 43 is not computed and counts 0 beside 42.  nIni = round(30 / 60) = 1
    "width 62": case("w62", [(42, 40, 130), (43, 40, 130)], [(42, 40, 0, 29)], fell=1, size=(62, 92)),
    "a single cell row": case("h62", [(40, 42, 130), (40, 43, 130)], [(40, 42, 0, 29)], fell=1, size=(92, 62)),
    # width = 61: wCell = 31, the second cell ends at 16 + 31 + 37 = 84, clamped to 77: x in [50, 74)
    "last cell clamped": case("w93", [(73, 40, 130), (74, 40, 130)], [(73, 40, 0, 29)], fell=3, size=(93, 92)),
    # width = 781: nCols = 26, wCell = 31; the last column starts at 16 + 775 = 791 >= 797 - 6 and is skipped (:775): 50 cells left,
    # one of them holds the corner.  nIni = round(781 / 60) = 13
    "last column skipped": case("w813", [(793, 40, 130), (794, 40, 130)], [(793, 40, 0, 29)], fell=49, size=(813, 92)),
    # height = 781: the last row starts at 791 < 797 - 3, is 6 px tall and computes nothing; 26 x 14 cells, all but one redone
    "last row 6 px tall": case("h813", [(100, 793, 130), (100, 794, 130)], [(100, 793, 0, 29)], fell=363, size=(470, 813)),
    # height = 871: nRows = 29, hCell = 31; the last row starts at 16 + 868 = 884 >= 887 - 3 and is skipped (:767): 28 x 14 cells
    "last row skipped": case("h903", [(100, 883, 130), (100, 884, 130)], [(100, 883, 0, 29)], fell=391, size=(470, 903)),
    # ---- the octree (dots at octree coordinates; candidates in cell order)
    # N of 0 and 1: the first sweep always runs and leaves n4, n1
    "N = 0": case("oct", rel((10, 10), (40, 40)), [(56, 56, 0, 29), (26, 26, 0, 29)], cand=[(26, 26, 29), (56, 56, 29)], fell=2, nfeatures=0),
    "N = 1": case("oct", rel((10, 10), (40, 40)), [(56, 56, 0, 29), (26, 26, 0, 29)], cand=[(26, 26, 29), (56, 56, 29)], fell=2, nfeatures=1),
    "N = 1, one key": case("oct", rel((10, 10)), [(26, 26, 0, 29)], fell=3, nfeatures=1),
    # nIni = 2 (152 x 92): the two initial nodes keep their order, there is no sweep that reverses them
    "nIni = 2": case("oct152", rel((10, 10), (70, 10)), [(26, 26, 0, 29), (86, 26, 0, 29)], fell=6, size=(152, 92)),
    # one node, two keys of one response: the first; of two responses: the larger
    "response tie in a node": case("oct", rel((10, 10), (14, 10)), [(26, 26, 0, 29)], cand=[(26, 26, 29), (30, 26, 29)], fell=3, nfeatures=1),
    "larger response behind": case("oct", rel((10, 10), (14, 10, 131)), [(30, 26, 0, 30)], cand=[(26, 26, 29), (30, 26, 30)], fell=3, nfeatures=1),
    # a b c in n1's quadrants 1 2 3, d e in n4.  Sweep 1 leaves [n4, n1], nToExpand = 2.
    # N = 2: reached by the sweep: e (the larger of n4), a (the first of n1)
    "N reached by the sweep": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)), [(66, 66, 0, 39), (21, 21, 0, 29)],
                                   cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=2),
    # N = 3: 2 + 3 x 2 > 3, phase 2 divides n1 (3 keys) first: [c, b, a, n4], size 4 >= 3 (reached by + 1)
    "phase 2, N passed by one": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)),
                                     [(21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29), (66, 66, 0, 39)],
                                     cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=3),
    "phase 2, N reached exactly": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)),
                                       [(21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29), (66, 66, 0, 39)],
                                       cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=4),
    # N = 5: n4 is divided too: [e, d, c, b, a]
    "phase 2, both divided": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)),
                                  [(66, 66, 0, 39), (56, 56, 0, 29), (21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29)],
                                  cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=5),
    # N = 7: 2 + 3 x 2 = 8 is one above N, so phase 2 it is: n1 first, then n4: [e, d, c, b, a]; nothing is left to divide (:710).
    # N = 8 below: 8 > 8 fails, a second SWEEP runs instead and leaves another order
    "phase-2 switch one above N": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)),
                                       [(66, 66, 0, 39), (56, 56, 0, 29), (21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29)],
                                       cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=7),
    # N = 8 is never reached: 2 + 6 <= 8, so a second SWEEP divides both (n1 first, the list's order is [n4, n1]: n4's children are
    # created first): [c, b, a, e, d]; five single keys, the next sweep changes nothing (:649)
    "N never reached": case("oct", rel((5, 5), (20, 5), (5, 20), (40, 40), (50, 50, 140)),
                            [(21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29), (66, 66, 0, 39), (56, 56, 0, 29)],
                            cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=8),
    # n1 and n4 hold two keys each, N = 3: the declared tie - n4, created last, is divided first: [e, d, n1], and n1 gives its first key
    "two equal sizes in phase 2": case("oct", rel((5, 5), (20, 5), (40, 40), (50, 50, 140)), [(66, 66, 0, 39), (56, 56, 0, 29), (21, 21, 0, 29)],
                                       cand=[(21, 21, 29), (36, 21, 29), (56, 56, 29), (66, 66, 39)], fell=2, nfeatures=3),
    # 93 x 92: the root is [0, 61) and its half ceil(30.5) = 31, so a (x = 30) is alone in n1, b in n2, c in n4: [c, b, a]
    "floor for ceil": case("w93", rel((30, 10), (45, 10), (40, 40)), [(56, 56, 0, 29), (61, 26, 0, 29), (46, 26, 0, 29)],
                           cand=[(46, 26, 29), (61, 26, 29), (56, 56, 29)], fell=1, size=(93, 92)),
    # n1 holds a b c d in its four quadrants, n4 holds e.  Sweep 1 leaves [n4, n1], size 2 = N - 1, nToExpand = 1, 2 + 3 > 3: phase 2 divides
    # n1 into four: size 5 = N + 2, the level's bound max(N + 2, 4 nIni), which is also the output capacity the case runs with
    "phase 2, N passed by two": case("oct", rel((5, 5), (20, 5), (5, 20), (20, 20), (40, 40)),
                                     [(36, 36, 0, 29), (21, 36, 0, 29), (36, 21, 0, 29), (21, 21, 0, 29), (56, 56, 0, 29)],
                                     cand=[(21, 21, 29), (36, 21, 29), (21, 36, 29), (36, 36, 29), (56, 56, 29)], fell=2, nfeatures=3, N=5),
    # 62 x 92: the root is [0, 30) x [0, 60).  P (14, 8) and Q (14, 10) travel together: [0, 15) x [0, 30) -> [8, 15) x [0, 15) -> [12, 15) x
    # [8, 15) -> [14, 15) x [8, 12), ONE pixel wide, which is divided at y = 10 (its x half is ceil(1 / 2) = 1: both keys lie left of 15).  H0 ..
    # H3 = (20, 40) (4, 4) (9, 4) (12, 9) drop out one per sweep, so the list grows 2 3 4 5 6 and no stop test holds before: [Q, P, H3, H2, H1, H0]
    "a node one pixel wide": case("w62", rel((14, 8), (14, 10), (20, 40), (4, 4), (9, 4), (12, 9)),
                                  [(30, 26, 0, 29), (30, 24, 0, 29), (28, 25, 0, 29), (25, 20, 0, 29), (20, 20, 0, 29), (36, 56, 0, 29)],
                                  cand=[(20, 20, 29), (25, 20, 29), (30, 24, 29), (28, 25, 29), (30, 26, 29), (36, 56, 29)], fell=0, size=(62, 92)),
    # 259 x 64: width 227, height 32, nIni = 7, hX = (float)(227 / 7) = 32.42856979..., below 227 / 7.  The last node's right edge is
    # (int)(hX * 7.0f) = (int)226.99998 = 226 where the rational value is 227; its left edge (int)(hX * 6.0f) = 194.  So the node is 32 wide
    # and its half ceil(32 / 2) = 16 puts the split at 210: the key at 210 goes RIGHT and the list becomes [n2, n1].  With the rational edge the
    # node is 33 wide, the split is at 211, both keys go left, the list keeps its size and ONE key comes out.  Both keys: (int)(x / hX) = 6
    "float node edge below the rational": case("w259", rel((200, 8), (210, 8)), [(226, 24, 0, 29), (216, 24, 0, 29)],
                                                 cand=[(216, 24, 29), (226, 24, 29)], fell=5, size=(259, 64)),
    # ---- capacities
    "cand_cap at the need": case("cap2", rel((10, 10), (40, 40)), [(56, 56, 0, 29), (26, 26, 0, 29)], cand=[(26, 26, 29), (56, 56, 29)], fell=2, cand_cap=2),
    "cand_cap one below the need": case("cap1", rel((10, 10), (40, 40)), [], cand=[(26, 26, 29)], fell=2, cand_cap=1, mask=1),
    # ---- an empty level behind a level with a corner (two levels: N_0 = cvRound(50 x (1 - 1/1.2) / (1 - 1/1.44)) = cvRound(27.27) = 27)
    "an empty level": case("two", None, [(40, 40, 0, 29)], fell=4, levels=[flat(92, 92, [(40, 40, 130)]), flat(77, 77)]),
}
CAND_TOTAL = {"cand_cap one below the need": 2}  # stat[0] counts the candidates found, whether they fit or not

# ---- the resize.  scale_factor 2: every coefficient is 1024 / 1024 (fx = 0.5), so a pixel is the mean of its 2 x 2 block, which for
# I(x, y) = 10 x is 20 dx + 5: r = 1024 (40 dx + 10), (r >> 4) = 64 (40 dx + 10), 2 x ((1024 x 64 (40 dx + 10)) >> 16) = 80 dx + 20,
# (80 dx + 22) >> 2 = 20 dx + 5.  Sizes on a half: cvRound(2.5) = 2, cvRound(3.5) = 4 (half to even).  scale_factor 1: fx = dx, so
# the last column and row meet the clamp sx >= sw - 1 and the level is a copy.
# Coefficients on a half: 2049 -> 2048 columns and rows (scale_factor 2049 / 2048, a float) give fx = dx + (2 dx + 1) / 4096 exactly, so
# sx = dx and fx x 2048 = dx + 0.5 in EVERY column: a1 = cvRound(dx + 0.5) is dx for even dx and dx + 1 for odd dx (half to even), a0 =
# cvRound(2047.5 - dx) = 2048 - a1; the same in y.  The pixel follows from the declared shifts; the coefficients are no powers of two and
# the row sums' low four bits are set, so `>> 4` dropped shows as well.
def _half_image():
    y, x = np.mgrid[0:2049, 0:2049]
    return ((x * 97 + y * 57 + 13) % 256).astype(np.uint8)


def _half_declared(l, h, w):
    if l == 0:
        return None
    S = _half_image().astype(np.int64)
    d = np.arange(2048)
    a1 = d + (d & 1)
    a0 = 2048 - a1
    r = a0 * S[:, d] + a1 * S[:, d + 1]  # 2049 rows
    r0, r1 = r[d], r[d + 1]
    b0, b1 = a0[:, None], a1[:, None]
    return ((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


RESIZE = {
    "coefficients on a half": dict(image=_half_image(), nlevels=2, scale_factor=2049.0 / 2048.0, sizes=[(2049, 2049), (2048, 2048)], declared=_half_declared),
    "constant": dict(image=np.full((37, 53), 201, np.uint8), nlevels=4, scale_factor=1.2, sizes=[(37, 53), (31, 44), (26, 37), (21, 31)],
                     declared=lambda l, h, w: np.full((h, w), 201, np.uint8)),
    "ramp halved": dict(image=np.tile(10 * np.arange(12, dtype=np.uint8), (8, 1)), nlevels=2, scale_factor=2.0, sizes=[(8, 12), (4, 6)],
                        declared=lambda l, h, w: np.tile((20 * np.arange(w) + 5).astype(np.uint8), (h, 1)) if l else None),
    "sizes on a half": dict(image=np.full((7, 5), 9, np.uint8), nlevels=2, scale_factor=2.0, sizes=[(7, 5), (4, 2)],
                            declared=lambda l, h, w: np.full((h, w), 9, np.uint8)),
    "the upper clamp": dict(image=(np.arange(35, dtype=np.uint8) * 7).reshape(5, 7), nlevels=2, scale_factor=1.0, sizes=[(5, 7), (5, 7)],
                            declared=lambda l, h, w: (np.arange(35, dtype=np.uint8) * 7).reshape(5, 7)),
}


def detect_groups():
    g = {}
    for name, c in DETECT.items():
        g.setdefault(c["group"], []).append(name)
    return g


def check_declared(name, got):
    """got: one image's outputs in the call's layout (or the model's, see as_call) against the case's declared ones"""
    c = DETECT[name]
    n = len(c["kp"])
    assert int(got["n_kp"]) == n, (name, int(got["n_kp"]), n)
    kp = np.array(c["kp"], np.int64).reshape(-1, 4)
    assert np.array_equal(got["kp_xy"][:n], kp[:, :2]) and np.array_equal(got["kp_oct"][:n], kp[:, 2]), (name, got["kp_xy"][:n], got["kp_oct"][:n])
    assert np.array_equal(got["kp_response"][:n], kp[:, 3].astype(np.float32)), (name, got["kp_response"][:n])
    assert np.all(got["kp_xy"][n:] == -1) and np.all(got["kp_oct"][n:] == -1) and np.all(got["kp_response"][n:] == 0), name
    cand = [(x, y, r) for x, y, _, r in c["kp"]] if c["cand"] is None else c["cand"]
    total = CAND_TOTAL.get(name, len(cand))
    assert list(got["cand_count"]) == [total] + [0] * 7, (name, got["cand_count"])
    m = len(cand)
    ca = np.array(cand, np.int64).reshape(-1, 3)
    assert np.array_equal(got["cand_xy"][0, :m], ca[:, :2]) and np.array_equal(got["cand_resp"][0, :m], ca[:, 2].astype(np.float32)), (name, got["cand_xy"][0, :m + 1])
    assert np.all(got["cand_xy"][0, m:] == -1) and np.all(got["cand_xy"][1:] == -1), name
    assert list(got["stat"]) == [total, c["fell"], n, c["mask"]], (name, got["stat"])
    assert int(got["level_count"].sum()) == n, name


def check_declared_resize(name, levels):
    c = RESIZE[name]
    assert [l.shape for l in levels] == c["sizes"], (name, [l.shape for l in levels])
    for l, img in enumerate(levels):
        want = c["declared"](l, *img.shape)
        assert want is None or np.array_equal(img, want), (name, l, img)
