"""Hand-built cases of Frame::computeStereoMatches (frame.cpp:179-349), one on each side of every decision, with every output DECLARED
here - worked out by hand from the reference's text, not taken from the model (tests/stereo_ref.py) or the device.  Test
infrastructure; nothing in the product imports it.

Every case is one frame on the same geometry, so that the cases also run as one batch: five levels, EVERY level image 64 x 48 (the
function only indexes a level image at the scaled coordinates; that a pyramid shrinks is the extractor's business), camera fx 32, bf 16
(mbf = 16, mb = 0.5, maxD = 32), 128 rows, scale factor 1.2.

How an image is made so that its SADs can be worked out by hand.  The images are black but for DOTS on the row BELOW a window's centre
row, so every window's centre value is 0 and the distance of two windows is the plain sum of |a - b|.  A left feature at level
coordinates (cx, cy) gets one dot of 100 at (cx, cy + 1).  A right dot of value q at column x on that row gives, for the right window
centred at column c (|x - c| <= 5): |100 - q| if x == c, else 100 + q; a window that does not hold the dot: 100.  So with the dot at the
key-point's own column cr the slide finds SAD = 100 - q at incR = 0, 100 + q on both sides (deltaR = 0, bestuR = sf[l] * cr), and
q = 100 - sad sets the SAD.  Descriptors: the left one is zero, a right one has `bits` ones - their distance.

A case up to :261 needs no image: on black images every SAD is 0, the first strict minimum is incR = -5 and the feature leaves at :306;
what the decision did shows in stat[0], the number of features that pass :261."""
import numpy as np

f32 = np.float32
CAM = (32.0, 16.0, 128)  # fx, bf, rows
SCALE = 1.2
NLEVELS, W, H = 5, 64, 48
SF = [f32(1.0)]  # frame::scale_factors: float, repeated multiply
for _ in range(7):
    SF.append(f32(SF[-1] * f32(1.2)))
MBF = f32(16.0)

CASES = {}


def bits(n):
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d)


def make(name, lefts, rights, dots_left=(), dots_right=(), n_left=None, n_right=None):
    """lefts: (u, v, octave); rights: (u, v, octave, bits); dots: (level, x, y, value)"""
    pl = [np.zeros((H, W), np.uint8) for _ in range(NLEVELS)]
    pr = [np.zeros((H, W), np.uint8) for _ in range(NLEVELS)]
    for img, dots in ((pl, dots_left), (pr, dots_right)):
        for l, x, y, v in dots:
            img[l][y, x] = v
    frame = dict(feat_uv=np.array([(u, v) for u, v, _ in lefts], np.float64).reshape(-1, 2), feat_oct=np.array([o for _, _, o in lefts], np.int32),
                 feat_desc=np.zeros((len(lefts), 32), np.uint8), r_uv=np.array([(u, v) for u, v, _, _ in rights], np.float32).reshape(-1, 2),
                 r_oct=np.array([o for _, _, o, _ in rights], np.int32), r_desc=np.array([bits(b) for _, _, _, b in rights], np.uint8).reshape(-1, 32),
                 pyr_left=pl, pyr_right=pr, n_left=n_left, n_right=n_right)
    assert name not in CASES
    CASES[name] = {"frame": frame}
    return CASES[name]


def expect(case, stat, matched=None, reset=()):
    """matched: {left feature: (right index, sad, u_right, depth)}; reset: those of them the median rule sets back to -1 / -1"""
    n = len(case["frame"]["feat_oct"])
    e = dict(feat_ur=np.full(n, -1.0, f32), feat_depth=np.full(n, -1.0, f32), match_r=np.full(n, -1, np.int32), sad=np.full(n, -1, np.int32),
             stat=np.array(stat, np.int32))
    for i, (r, s, ur, depth) in (matched or {}).items():
        e["match_r"][i], e["sad"][i] = r, s
        if i not in reset:
            e["feat_ur"][i], e["feat_depth"][i] = f32(ur), f32(depth)
    case["expect"] = e


def probe(name, left, rights, n261, **kw):
    """a case that ends at :306 on black images: stat = {n261, 0, 0, -1}, every feature -1"""
    lefts = left if isinstance(left, list) else [left]
    expect(make(name, lefts, rights, **kw), [n261, 0, 0, -1])


def below(x):
    return float(np.nextafter(f32(x), f32(-1e9)))


def above(x):
    return float(np.nextafter(f32(x), f32(1e9)))


# ---- the row band (:198-204).  Octave 0: r = 2; kpY = 18.5: minr = floor(16.5) = 16, maxr = ceil(20.5) = 21
for row, v, n in ((15, 15.5, 0), (16, 16.0, 1), (21, 21.99, 1), (22, 22.0, 0)):
    probe("band_oct0_row%d" % row, (40.0, v, 0), [(36.0, 18.5, 0, 10)], n)
# octave 3: r = 2 x 1.7280002 = 3.4560003; kpY = 40.5: minr = floor(37.044) = 37, maxr = ceil(43.956) = 44
for row, n in ((36, 0), (37, 1), (44, 1), (45, 0)):
    probe("band_oct3_row%d" % row, (40.0, row + 0.25, 3), [(36.0, 40.5, 3, 10)], n)
# kpY + r an exact integer: octave 0, kpY = 18: maxr = ceil(20.0) = 20, minr = 16
for row, n in ((15, 0), (16, 1), (20, 1), (21, 0)):
    probe("band_exact_row%d" % row, (40.0, row + 0.5, 0), [(36.0, 18.0, 0, 10)], n)
# ... and an integer only AS A FLOAT: octave 1, r = 2.4000001; kpY = 17.6f = 17.60000038: the sum 20.00000048 is nearer to 20.0 than to the
# next float (20.0000019), so maxr = 20 - in double it would be 21
probe("band_float_sum_row20", (40.0, 20.5, 1), [(36.0, 17.6, 1, 10)], 1)
probe("band_float_sum_row21", (40.0, 21.5, 1), [(36.0, 17.6, 1, 10)], 0)
# the left row truncates (:223): vL = 10.99 -> row 10; kpY = 8: rows 6 .. 10
probe("row_truncates_10_99", (40.0, 10.99, 0), [(36.0, 8.0, 0, 10)], 1)
probe("row_11_00", (40.0, 11.0, 0), [(36.0, 8.0, 0, 10)], 0)

# ---- the octave window (:244): levelL = 2
for o, n in ((0, 0), (1, 1), (2, 1), (3, 1), (4, 0)):
    probe("octave_window_r%d" % o, (40.0, 30.0, 2), [(36.0, 30.0, o, 10)], n)

# ---- the horizontal range (:228-232, :249): uL = 40, maxD = 32: minU = 8, maxU = 40
probe("u_at_minU", (40.0, 18.0, 0), [(8.0, 18.0, 0, 10)], 1)
probe("u_below_minU", (40.0, 18.0, 0), [(below(8.0), 18.0, 0, 10)], 0)
probe("u_at_uL", (40.0, 18.0, 0), [(40.0, 18.0, 0, 10)], 1)
probe("u_above_uL", (40.0, 18.0, 0), [(above(40.0), 18.0, 0, 10)], 0)
probe("uL_negative", (-0.5, 18.0, 0), [(-1.0, 18.0, 0, 10)], 0)   # maxU < 0: skipped, although uR lies in [minU, maxU]
probe("uL_zero", (0.0, 18.0, 0), [(0.0, 18.0, 0, 10)], 1)         # maxU == 0 is not < 0

# ---- the descriptor distance (:234, :253, :261)
probe("dist_99", (40.0, 18.0, 0), [(36.0, 18.0, 0, 99)], 0)       # below the initial 100, not below 75
probe("dist_100", (40.0, 18.0, 0), [(36.0, 18.0, 0, 100)], 0)
probe("dist_74", (40.0, 18.0, 0), [(36.0, 18.0, 0, 74)], 1)
probe("dist_75", (40.0, 18.0, 0), [(36.0, 18.0, 0, 75)], 0)


def pair_dots(l, cx, cy, xr, q=90):
    """the left dot of a feature at (cx, cy) of level l and ONE right dot of value q at column xr"""
    return dict(dots_left=[(l, cx, cy + 1, 100)], dots_right=[(l, xr, cy + 1, q)])


# Two candidates at level 0, both on the strip of the same dot (column 26): from uR = 26 the slide finds it at incR = 0, from uR = 22 at
# incR = +4 (SAD 10, 190 on both sides) - bestuR = 26 either way, disparity 30 - 26 = 4, depth 16 / 4; only match_r tells who won.
c = make("dist_tie_lower_index_wins", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 30), (22.0, 18.0, 0, 30)], **pair_dots(0, 30, 18, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, 4.0)})
c = make("dist_later_smaller_wins", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 30), (22.0, 18.0, 0, 29)], **pair_dots(0, 30, 18, 26))
expect(c, [1, 1, 0, 10], {0: (1, 10, 26.0, 4.0)})

# ---- rounding (:265-267).  Level 0: uv.x = 30.5 -> 31 (half away from zero; half to even would say 30), 31.5 -> 32 (both rules).  The dot
# is at the rounded column, so the slide stays at incR = 0: uR = 26 -> bestuR = 26.
c = make("round_half_30_5", [(30.5, 18.0, 0)], [(26.0, 18.0, 0, 10)], **pair_dots(0, 31, 18, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, f32(16.0) / f32(4.5))})
c = make("round_half_31_5", [(31.5, 18.0, 0)], [(26.0, 18.0, 0, 10)], **pair_dots(0, 32, 18, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, f32(16.0) / f32(5.5))})
# The right key-point's product is a FLOAT product (found by search on the CPU): level 1, inv = 0.8333333134651184f, uR0 = 27:
# 27 x inv = 22.49999946... rounds to the float 22.5 -> 23; the double product stays below one half -> 22.  The dot is at column 27 =
# 23 + 4: incR = +4, bestuR = 1.2f x 27 (from 22 it would be incR = +5 and the feature would leave at :306).
# The left feature: uv = (36, 21.6) -> (round(29.9999993), round(17.9999996)) = (30, 18); row (int)21.6f = 21, inside 19 .. 25.
UR = f32(SF[1] * f32(27.0))
c = make("float_product_right", [(36.0, 21.6, 1)], [(27.0, 21.6, 1, 10)], **pair_dots(1, 30, 18, 27))
expect(c, [1, 1, 0, 10], {0: (0, 10, UR, MBF / f32(f32(36.0) - UR))})
# The left feature's product is a DOUBLE product: level 1, uv.x = 27: 22.49999946 -> 22 (as a float product 22.5 -> 23).  uR0 = 24 ->
# 19.9999995 -> 20 in either format; the dot at column 20: incR = 0, bestuR = 1.2f x 20.  (With the left window at 23 its dot would sit at
# offset -1 and the slide would answer incR = +1.)
UR = f32(SF[1] * f32(20.0))
c = make("double_product_left", [(27.0, 21.6, 1)], [(24.0, 21.6, 1, 10)], dots_left=[(1, 22, 19, 100)], dots_right=[(1, 20, 19, 90)])
expect(c, [1, 1, 0, 10], {0: (0, 10, UR, MBF / f32(f32(27.0) - UR))})

# ---- the window test (:284-287) and deviation 4.  Width 64.
c = make("endu_at_width_minus_1", [(58.0, 18.0, 0)], [(52.0, 18.0, 0, 10)], **pair_dots(0, 58, 18, 52))  # 52 + 11 = 63
expect(c, [1, 1, 0, 10], {0: (0, 10, 52.0, f32(16.0) / f32(6.0))})
c = make("endu_at_width", [(58.0, 18.0, 0)], [(53.0, 18.0, 0, 10)], **pair_dots(0, 58, 18, 53))          # 53 + 11 = 64: skipped
expect(c, [1, 0, 0, -1])
c = make("right_strip_from_column_0", [(20.0, 18.0, 0)], [(10.0, 18.0, 0, 10)], **pair_dots(0, 20, 18, 10))
expect(c, [1, 1, 0, 10], {0: (0, 10, 10.0, f32(16.0) / f32(10.0))})
c = make("scaleduR0_zero_deviation_4", [(20.0, 18.0, 0)], [(0.0, 18.0, 0, 10)], **pair_dots(0, 20, 18, 0))  # passes :286, first window at -10
expect(c, [1, 0, 0, -1])
c = make("scaleduR0_nine_deviation_4", [(20.0, 18.0, 0)], [(9.0, 18.0, 0, 10)], **pair_dots(0, 20, 18, 9))
expect(c, [1, 0, 0, -1])
# the left window on the image's edges: rows 0 .. 10 and 37 .. 47, columns .. 63; one further out is deviation 4
c = make("left_window_top_edge", [(30.0, 5.0, 0)], [(26.0, 5.0, 0, 10)], **pair_dots(0, 30, 5, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, 4.0)})
c = make("left_window_above_top", [(30.0, 4.0, 0)], [(26.0, 4.0, 0, 10)], **pair_dots(0, 30, 4, 26))
expect(c, [1, 0, 0, -1])
c = make("left_window_bottom_edge", [(30.0, 42.0, 0)], [(26.0, 42.0, 0, 10)], **pair_dots(0, 30, 42, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, 4.0)})
c = make("left_window_below_bottom", [(30.0, 43.0, 0)], [(26.0, 43.0, 0, 10)], **pair_dots(0, 30, 43, 26))
expect(c, [1, 0, 0, -1])
c = make("left_window_beyond_right_edge", [(59.0, 18.0, 0)], [(52.0, 18.0, 0, 10)], **pair_dots(0, 59, 18, 52))  # columns 54 .. 64
expect(c, [1, 0, 0, -1])
# (a left window on column 0 has uL = 5, so uR <= 5 and the right strip starts left of the image: it cannot match on either side)
c = make("left_window_left_edge", [(5.0, 18.0, 0)], [(5.0, 18.0, 0, 10)], **pair_dots(0, 5, 18, 5))
expect(c, [1, 0, 0, -1])

# ---- the SAD (:289-306).  A tie between incR = 0 and +1: dots of 90 at columns cr and cr + 1: SAD(0) = 10 + 90, SAD(+1) = 90 + 10,
# SAD(-1) = 100 + 90 + 90 = 280: the first wins; d1 = 280, d2 = d3 = 100: deltaR = 180 / (2 x 180) = +0.5; bestuR = 26.5, disparity 3.5
c = make("sad_tie_first_wins_delta_half", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 10)], dots_left=[(0, 30, 19, 100)],
         dots_right=[(0, 26, 19, 90), (0, 27, 19, 90)])
expect(c, [1, 1, 0, 100], {0: (0, 100, 26.5, f32(16.0) / f32(3.5))})
# a tie two steps apart: dots of 90 at cr and cr + 2: SAD(0) = SAD(+2) = 100, SAD(-1) = SAD(+1) = 280: the first wins, deltaR = 0, bestuR = 26
# (the later one would give 28)
c = make("sad_tie_two_apart_first_wins", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 10)], dots_left=[(0, 30, 19, 100)],
         dots_right=[(0, 26, 19, 90), (0, 28, 19, 90)])
expect(c, [1, 1, 0, 100], {0: (0, 100, 26.0, 4.0)})
# the best at incR = k: the dot at column cr + k; cr = 30, uL = 40
for k, m in ((-5, None), (-4, (0, 10, 26.0, f32(16.0) / f32(14.0))), (4, (0, 10, 34.0, f32(16.0) / f32(6.0))), (5, None)):
    c = make("sad_best_at_%+d" % k, [(40.0, 18.0, 0)], [(30.0, 18.0, 0, 10)], **pair_dots(0, 40, 18, 30 + k))
    expect(c, [1, 1, 0, 10] if m else [1, 0, 0, -1], {0: m} if m else None)
# the parabola with d1 - d2 == d3 - d2: deltaR = 0 (every plain pair above); asymmetric: dots 90 at cr, 20 at cr + 1: SAD(0) = 10 + 20 = 30,
# SAD(-1) = 100 + 90 + 20 = 210, SAD(+1) = 80 + 90 = 170: deltaR = 40 / (2 x (380 - 60)) = 0.0625; bestuR = 26.0625
c = make("parabola_asymmetric", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 10)], dots_left=[(0, 30, 19, 100)], dots_right=[(0, 26, 19, 90), (0, 27, 19, 20)])
expect(c, [1, 1, 0, 30], {0: (0, 30, 26.0625, f32(16.0) / f32(3.9375))})

# ---- the disparity (:323-331)
# exactly 0: uR = uL = 30: disparity becomes (float)0.01, bestuR = (float)(30.0 - 0.01)
c = make("disparity_zero", [(30.0, 18.0, 0)], [(30.0, 18.0, 0, 10)], **pair_dots(0, 30, 18, 30))
expect(c, [1, 1, 0, 10], {0: (0, 10, f32(29.99), MBF / f32(0.01))})
# bestuR = 30 one float above uL = 29.999998 (uR = 29.6 <= uL is a candidate, both round to column 30): disparity < 0, dropped
c = make("disparity_one_float_negative", [(below(30.0), 18.0, 0)], [(29.6, 18.0, 0, 10)], **pair_dots(0, 30, 18, 30))
expect(c, [1, 0, 0, -1])
# at maxD: uL = 58, bestuR = 26: 32 is not < 32; one float below: uL = 57.999996 (minU = 25.999996 <= 26)
c = make("disparity_at_maxD", [(58.0, 18.0, 0)], [(26.0, 18.0, 0, 10)], **pair_dots(0, 58, 18, 26))
expect(c, [1, 0, 0, -1])
c = make("disparity_below_maxD", [(below(58.0), 18.0, 0)], [(26.0, 18.0, 0, 10)], **pair_dots(0, 58, 18, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, MBF / f32(f32(below(58.0)) - f32(26.0)))})

# ---- the median rule (:337-348): features on rows 6, 18, 30, 41 (windows and bands apart), uL = 30, uR = 26, SAD s through q = 100 - s
ROWS = (6, 18, 30, 41)


def median_case(name, sads, stat, reset):
    n = len(sads)
    c = make(name, [(30.0, float(ROWS[i]), 0) for i in range(n)], [(26.0, float(ROWS[i]), 0, 10) for i in range(n)],
             dots_left=[(0, 30, ROWS[i] + 1, 100) for i in range(n)], dots_right=[(0, 26, ROWS[i] + 1, 100 - sads[i]) for i in range(n)])
    expect(c, stat, {i: (i, sads[i], 26.0, 4.0) for i in range(n)}, reset=reset)


# thDist = (1.5f x 1.4f) x median = 2.0999999f x median, e.g. 21.0 exactly for a median of 10
median_case("median_n1", [10], [1, 1, 0, 10], ())
median_case("median_n2", [10, 30], [2, 2, 0, 30], ())                 # position 1: 30 -> 63; (position 0 would reset the 30)
median_case("median_n3", [30, 10, 12], [3, 3, 1, 12], (0,))           # position 1: 12 -> 25.2: 30 is reset
median_case("median_n4", [32, 10, 30, 12], [4, 4, 0, 30], ())         # position 2: 30 -> 63; (position 1 would reset two)
median_case("median_sad_below_th", [10, 20, 10], [3, 3, 0, 10], ())   # thDist = 21.0
median_case("median_sad_on_th", [10, 21, 10], [3, 3, 1, 10], (1,))    # 21 >= 21.0
median_case("median_sad_above_th", [10, 22, 10], [3, 3, 1, 10], (1,))
median_case("median_all_equal", [10, 10, 10], [3, 3, 0, 10], ())
median_case("median_zero_resets_all", [0, 0], [2, 2, 2, 0], (0, 1))   # thDist = 0: exact matches included
median_case("median_zero_resets_all_n3", [0, 0, 50], [3, 3, 3, 0], (0, 1, 2))
probe("empty_list", (40.0, 18.0, 0), [(36.0, 18.0, 0, 80)], 0)        # deviation 5: nothing to take a median of

# ---- input handling
# deviation 1: rows of a band outside [0, 128) are dropped, the others count
probe("dev1_band_over_top", (40.0, 1.5, 0), [(36.0, 0.5, 0, 10)], 1)          # band -2 .. 3
probe("dev1_band_over_bottom", (40.0, 127.2, 0), [(36.0, 127.5, 0, 10)], 1)   # band 125 .. 130
probe("dev1_band_all_outside", (40.0, 0.5, 0), [(36.0, -5.0, 0, 10)], 0)      # band -7 .. -3
# deviation 2
probe("dev2_vL_negative", (40.0, -0.5, 0), [(36.0, 0.5, 0, 10)], 0)           # (size_t)-0.5f is not row 0
probe("dev2_vL_at_height", (40.0, 128.0, 0), [(36.0, 127.5, 0, 10)], 0)
# deviation 3
probe("dev3_left_octave_5", (40.0, 18.0, 5), [(36.0, 18.0, 4, 10)], 0)
probe("dev3_left_octave_negative", (40.0, 18.0, -1), [(36.0, 18.0, 0, 10)], 0)
probe("dev3_right_octave_5", (40.0, 18.0, 4), [(36.0, 18.0, 5, 10)], 0)
probe("dev3_right_octave_negative", (40.0, 18.0, 0), [(36.0, 18.0, -1, 10)], 0)
# padding: slots at or beyond a count join nothing
c = make("padding_n_left", [(30.0, 18.0, 0), (30.0, 30.0, 0)], [(26.0, 18.0, 0, 10), (26.0, 30.0, 0, 10)],
         dots_left=[(0, 30, 19, 100), (0, 30, 31, 100)], dots_right=[(0, 26, 19, 90), (0, 26, 31, 90)], n_left=1)
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, 4.0)})
c = make("padding_n_right", [(30.0, 18.0, 0)], [(26.0, 18.0, 0, 30), (22.0, 18.0, 0, 5)], n_right=1, **pair_dots(0, 30, 18, 26))
expect(c, [1, 1, 0, 10], {0: (0, 10, 26.0, 4.0)})   # (the better candidate is slot 1)
