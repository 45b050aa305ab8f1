"""A bit-exact host model of GL_ASSOC_SCREENED (gmmloc_amd/csrc/gl_assoc32.hip), in pure Python.  Test infrastructure for
tests/assoc_screen_cases.py, tests/test_assoc_screen_cases.py (CPU) and tests/test_gpu_assoc_screen_cases.py.

The screen promises the exhaustive sweep's idx and d2 for every input.  That rests on an fp32 error bound proved by hand and on the
bookkeeping of short candidate lists; for a given map and points the two counters GL_COUNTER_ASSOC_SCREEN_VERIFIED / _FALLBACK are
exact functions of both, so a model that restates the source operation for operation can declare them and the device must give them.

fp32 arithmetic: +, -, * in numpy.float32 round correctly; fmaf goes through fractions.Fraction and is rounded ONCE to fp32, ties to
even (round_f32; float32(float(Fraction)) would round twice).  The library is built with -ffp-contract=off, so the source's
expression order gives the bits.  fp64 arithmetic: Python floats, as in tests/assoc_model.py, whose record(), chi2_device() and
chi2_exact() this file uses.

  source_constants()      kCap, kOut, kLimit and the figures of THE BOUND, read from gl_assoc32.hip (and kChunk and the launch-shape
                          statements from gl_assoc.hip / gl_internal.hpp): a changed source is followed or flagged
  ScreenMap(mean, cov)    build_screen_records: o, rmax, cmax and the fp32 records, or records = None (map without a screen)
  screen_point(m, p)      screen_point: P, G, H, ok (mutation beta_zero: the beta term of the bound removed)
  pair(r, q)              screen_pair / screen_lo (one function: the same arithmetic): hi, lo, and every intermediate on request
  screen_shape(K, N)      screen_shape / sweep_split / sweep_points and the verify kernel's L
  screen_split(...)       one point through one K split of k_assoc_screen: chunks of 8, hmin / lmin, U, note() with its compaction,
                          the final filter to kOut with `lost`
  associate_point(...)    one point through both kernels: (idx, d2, verified, fell_back)

`strict` (the default for the declared cases): every fp32 intermediate must be zero or normal - a declared case must not depend on
how the device treats fp32 subnormals, nor on an infinity.
"""
import math
import os
import re
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np

from tests import assoc_model as am
from tests.assoc_model import record, chi2_device, chi2_exact  # noqa: F401  (re-exported: the fp64 side of every check)

f32 = np.float32
CSRC = os.path.join(am.ROOT, "gmmloc_amd", "csrc")
SCREEN_SRC = os.path.join(CSRC, "gl_assoc32.hip")
SWEEP_SRC = os.path.join(CSRC, "gl_assoc.hip")
INTERNAL_SRC = os.path.join(CSRC, "gl_internal.hpp")
F32_MIN_NORMAL = 2.0 ** -126
INF32 = f32(np.inf)


# ---- fp32 ------------------------------------------------------------------------------------------------------------------------------
def round_f32(x):
    """the Fraction x rounded once to fp32, ties to even (subnormals and overflow to infinity included)"""
    if x == 0:
        return f32(0.0)
    neg = x < 0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if (n if e >= 0 else n << -e) < (d << e if e >= 0 else d):
        e -= 1  # now 2^e <= |x| < 2^(e + 1)
    q = max(e, -126) - 23  # the exponent of the last place
    num, den = (n, d << q) if q >= 0 else (n << -q, d)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    v = math.ldexp(m, q) if q < 200 else math.inf  # m <= 2^24: exact in a double
    if v >= 2.0 ** 128:
        v = math.inf
    return f32(-v if neg else v)


def fmaf(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return f32(a * b + c)  # an infinity or a NaN either way
    x = Fr(a) * Fr(b) + Fr(c)
    if x == 0:  # the sign of an exact zero: -0 only if both the product and the addend are -0
        pneg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0
        return f32(-0.0) if pneg and math.copysign(1.0, c) < 0 else f32(0.0)
    return round_f32(x)


def nudged(v, ulps):
    for _ in range(abs(ulps)):
        v = np.nextafter(v, INF32 if ulps > 0 else -INF32)
    return v


# ---- the constants, from the source ---------------------------------------------------------------------------------------------------
_constants = None


def source_constants():
    global _constants
    if _constants is None:
        src, swp, hdr = open(SCREEN_SRC).read(), open(SWEEP_SRC).read(), open(INTERNAL_SRC).read()

        def one(pat, text=src, conv=float):
            m = re.findall(pat, text)
            assert len(m) == 1, (pat, m)
            return tuple(conv(v) for v in m[0]) if isinstance(m[0], tuple) else conv(m[0])
        num, hx = r"([0-9.]+(?:e[+-]?[0-9]+)?)", r"(0x1p-?[0-9]+)"
        c = dict(kCap=one(r"constexpr int kCap = ([0-9]+);", conv=int), kOut=one(r"constexpr int kOut = ([0-9]+);", conv=int),
                 kLimit=one(r"constexpr float kLimit = " + num + "f;"), kChunk=one(r"constexpr int kChunk = ([0-9]+);", swp, int))
        c["beta_u"], c["beta_floor"] = one(r"const double beta = " + num + r" \* 0x1p-24 \* L \+ " + num + ";")
        g = one(r"const double G = " + hx + r" \+ " + num + r" \* beta, F = " + num + r" \* beta \+ " + num + r" \* beta \* beta, H = F / G;", conv=str)
        c["G0"], c["G1"], c["F1"], c["F2"] = float.fromhex(g[0]), float(g[1]), float(g[2]), float(g[3])
        c["up"] = one(r"const double up = 1\.0 \+ " + hx + ";", conv=float.fromhex)
        c["big"] = one(r"const double big = g\.cmax \* \(" + num + r" \* L \* L \+ H\) \* \(1\.0 \+ G\);")
        cm = one(r"c = std::max\(c \* \(1\.0 \+ " + hx + r"\), " + num + r"\);", conv=str)
        c["c_up"], c["c_floor"] = float.fromhex(cm[0]), float(cm[1])
        c["rmax_up"] = one(r"g->scr_rmax = rmax \* \(1\.0 \+ " + num + r"\);")
        c["map_limit"] = one(r"cmax \* \(g->scr_rmax \* g->scr_rmax\) < " + num + ";")
        # the statements restated below without a figure of their own to read: flagged if they change
        for text, stmt in ((src, "const int ppt = gl::sweep_points(N, listed) >= 16384 ? 4 : 2;"),
                           (src, "while (4 * L < nsplit && L < 16) L <<= 1;"),
                           (src, "constexpr int PPT = 2 * NP, CAP = kCap / NP, ST = PPT * 256;"),
                           (src, "const int k1 = min(geo.K, k0 + 8);"),
                           (src, "for (int k0 = k_begin; k0 < k_end; k0 += 8) {"),
                           (hdr, "inline int sweep_points(int N, bool listed) { return listed ? (N / 16 > 256 ? N / 16 : 256) : N; }"),
                           (swp, "const int target_blocks = (Ne >= 8192) ? 4096 : (listed ? 1024 : 512);"),
                           (swp, "const int max_split = (K + 63) / 64;"),
                           (swp, "const int etiles = (Ne + 256 * ppt - 1) / (256 * ppt);")):
            assert stmt in text, stmt
        assert c["kChunk"] == 8  # the screen's chunks of 8 are the sweep's
        _constants = c
    return _constants


# ---- build_screen_records ------------------------------------------------------------------------------------------------------------
class ScreenMap:
    """what gl_gmm_create keeps for the screen: the fp64 records, the origin o, rmax, cmax and the fp32 records r32 (a list of 10
    float32 per component), or r32 = None where build_screen_records gives the map no screen records"""

    def __init__(self, mean, cov):
        c = source_constants()
        self.mean, self.cov = np.asarray(mean, np.float64), np.asarray(cov, np.float64).reshape(-1, 9)
        self.rec = [record(m, cv) for m, cv in zip(self.mean, self.cov)]
        self.K = K = len(self.rec)
        lo, hi = list(self.rec[0][:3]), list(self.rec[0][:3])
        ok = True
        for r in self.rec:
            for a in range(3):
                ok = ok and math.isfinite(r[a])
                lo[a], hi[a] = min(lo[a], r[a]), max(hi[a], r[a])
        self.o = [0.5 * lo[a] + 0.5 * hi[a] for a in range(3)]
        r32, rmax, cmax = [], 0.0, 0.0
        with np.errstate(all="ignore"):
            for r in self.rec:
                if not ok:
                    break
                A = r[3:]
                cc = 0.0
                for i in range(3):
                    row = abs(A[i * 3]) + abs(A[i * 3 + 1]) + abs(A[i * 3 + 2])
                    col = abs(A[i]) + abs(A[3 + i]) + abs(A[6 + i])
                    cc = max(cc, max(row, col)) if row == row and col == col else math.nan
                cc = max(cc * (1.0 + c["c_up"]), c["c_floor"]) if cc == cc else math.nan
                w = []
                for a in range(3):
                    d = r[a] - self.o[a]
                    rmax = max(rmax, abs(d))
                    w.append(f32(d))
                w += [f32(A[0]), f32(A[4]), f32(A[8]), f32(A[1] + A[3]), f32(A[2] + A[6]), f32(A[5] + A[7]), f32(cc)]
                if float(w[9]) > cmax:
                    cmax = float(w[9])
                ok = ok and all(math.isfinite(float(v)) for v in w)
                r32.append(w)
        self.rmax = rmax * (1.0 + c["rmax_up"])
        self.cmax = cmax
        ok = ok and math.isfinite(self.rmax) and cmax * (self.rmax * self.rmax) < c["map_limit"]
        self.r32 = r32 if ok else None


# ---- screen_point ----------------------------------------------------------------------------------------------------------------------
Pt = namedtuple("Pt", "P G H ok rho beta Gd Hd big")


def screen_point(m, p, beta_zero=False):
    c = source_constants()
    x, y, z = (float(v) for v in p)
    with np.errstate(all="ignore"):
        dx, dy, dz = x - m.o[0], y - m.o[1], z - m.o[2]
        ab = [abs(v) for v in (dx, dy, dz) if v == v]  # fmax ignores a NaN
        rho = max(ab) if ab else math.nan
        L = rho + m.rmax
        beta = 0.0 if beta_zero else c["beta_u"] * 2.0 ** -24 * L + c["beta_floor"]
        G = c["G0"] + c["G1"] * beta
        F = c["F1"] * beta + c["F2"] * beta * beta
        H = F / G
        up = 1.0 + c["up"]
        big = m.cmax * (c["big"] * L * L + H) * (1.0 + G)
        ok = x == x and y == y and z == z and big <= float(f32(c["kLimit"]))
        return Pt((f32(dx), f32(dy), f32(dz)), f32(G * up), f32(H * up), bool(ok), rho, beta, G, H, big)


# ---- screen_pair / screen_lo -----------------------------------------------------------------------------------------------------------
STAGES = ("d0", "d1", "d2", "t0a", "t0b", "t0", "t1a", "t1", "t2", "s0", "s1", "s", "n0", "n1", "n", "E", "hi", "lo")


class Subnormal(AssertionError):
    pass


def pair(r, q, strict=True, nudge=None, trace=None):
    """hi, lo of one fp32 record r for the point q: screen_pair for one half of the packed pair, and screen_lo (its lo).
    nudge = {stage: ulps}: that intermediate moved by so many fp32 ulps (to ask which rounding decides a case);
    trace: a dict that receives every intermediate."""
    def R(name, v):
        if nudge and name in nudge:
            v = nudged(v, nudge[name])
        if strict:
            a = abs(float(v))
            if not (a == 0.0 or (F32_MIN_NORMAL <= a < math.inf)):
                raise Subnormal("%s = %r is neither zero nor a normal fp32 number" % (name, v))
        if trace is not None:
            trace[name] = v
        return v
    with np.errstate(all="ignore"):
        d0, d1, d2 = R("d0", q.P[0] - r[0]), R("d1", q.P[1] - r[1]), R("d2", q.P[2] - r[2])
        t0 = R("t0", fmaf(d2, r[7], R("t0b", fmaf(d1, r[6], R("t0a", d0 * r[3])))))
        t1 = R("t1", fmaf(d2, r[8], R("t1a", d1 * r[4])))
        t2 = R("t2", d2 * r[5])
        s = R("s", fmaf(d2, t2, R("s1", fmaf(d1, t1, R("s0", t0 * d0)))))
        n = R("n", fmaf(d2, d2, R("n1", fmaf(d1, d1, R("n0", fmaf(d0, d0, q.H))))))
        E = R("E", n * r[9])
        return R("hi", fmaf(E, q.G, s)), R("lo", fmaf(-E, q.G, s))


# ---- the launch shape ------------------------------------------------------------------------------------------------------------------
def sweep_points(N, listed=False):
    return (N // 16 if N // 16 > 256 else 256) if listed else N


def sweep_split(K, N, listed, ppt):
    kc = source_constants()["kChunk"]
    Ne = sweep_points(N, listed)
    etiles = (Ne + 256 * ppt - 1) // (256 * ppt)
    target = 4096 if Ne >= 8192 else (1024 if listed else 512)
    nsplit = min((target + etiles - 1) // etiles, (K + 63) // 64)
    nsplit = max(nsplit, 1)
    kchunk = (K + nsplit - 1) // nsplit
    kchunk = (kchunk + kc - 1) // kc * kc
    return (N + 256 * ppt - 1) // (256 * ppt), (K + kchunk - 1) // kchunk, kchunk


def screen_shape(K, N, listed=False):
    """dict(ppt, ptiles, nsplit, kchunk, chunks: chunks per full split, cap: list entries per point, L: verify lanes per point)"""
    c = source_constants()
    ppt = 4 if sweep_points(N, listed) >= 16384 else 2
    ptiles, nsplit, kchunk = sweep_split(K, N, listed, ppt)
    L = 1
    while 4 * L < nsplit and L < 16:
        L <<= 1
    return dict(ppt=ppt, ptiles=ptiles, nsplit=nsplit, kchunk=kchunk, chunks=(min(kchunk, K) + 7) // 8,
                cap=c["kCap"] // (ppt // 2), L=L)


# ---- k_assoc_screen, one point and one split -------------------------------------------------------------------------------------------
Split = namedtuple("Split", "U lost out compactions peak")


def screen_split(los_his, k_begin, k_end, cap, kout, compact_drops_equal=False):
    """los_his(k) -> (hi, lo).  Returns U, lost, the (k0, lo) handed to the verify kernel, how often note() compacted and the longest
    the list ever was.  Mutation compact_drops_equal: the compaction keeps l < U instead of !(l > U)."""
    U, lost = INF32, INF32
    lst = []
    compactions = peak = 0
    for k0 in range(k_begin, k_end, 8):
        hmin = lmin = None
        for k in range(k0, min(k0 + 8, k_end)):
            hi, lo = los_his(k)
            hmin = hi if hmin is None else np.minimum(hmin, hi)
            lmin = lo if lmin is None else np.minimum(lmin, lo)
        U = np.minimum(U, hmin)
        if not (lmin > U):  # note(p, k0, lmin)
            if len(lst) == cap:
                compactions += 1
                lst = [(k, l) for k, l in lst if (l < U if compact_drops_equal else not (l > U))]
            if len(lst) < cap:
                lst.append((k0, lmin))
            else:
                lost = np.minimum(lost, lmin)
            peak = max(peak, len(lst))
    out = []
    for k0, l in lst:
        if l > U:
            continue
        if len(out) < kout:
            out.append((k0, l))
        else:
            lost = np.minimum(lost, l)
    return Split(U, lost, out, compactions, peak)


# ---- both kernels, one point -----------------------------------------------------------------------------------------------------------
Result = namedtuple("Result", "idx d2 verified fell_back U splits")


def exhaustive(m, p, memo=None):
    """k_assoc_brute + k_assoc_merge: the first strict minimum of chi2_device in ascending k (-1, +inf if every chi2 is NaN)"""
    best, bi = math.inf, -1
    for k, r in enumerate(m.rec):
        v = chi2_device(r, p)
        if memo is not None:
            memo[k] = v
        if v < best:
            best, bi = v, k
    return bi, best


def associate_point(m, p, N, listed=False, beta_zero=False, retest_strict=False, compact_drops_equal=False, strict=True, nudge=None,
                    reference=None):
    """One point of an N-point call through k_assoc_screen and k_assoc_screen_verify.
    Mutations: beta_zero (screen_point), retest_strict (the verify kernel skips a component at lo >= U instead of lo > U),
    compact_drops_equal (screen_split).  nudge = (k, {stage: ulps}) for pair() of component k.
    reference = (idx, d2) of the fp64 sweep for this point if the caller has it (a fallen-back point returns it)."""
    c = source_constants()
    K = m.K
    fb_answer = (lambda: reference if reference is not None else exhaustive(m, p))
    if m.r32 is None:
        return Result(*fb_answer(), 0, True, None, [])
    sh = screen_shape(K, N, listed)
    q = screen_point(m, p, beta_zero)
    if not q.ok:  # U and the lists are still made on the device, and nothing reads them
        return Result(*fb_answer(), 0, True, None, [])
    cache = {}

    def hl(k):
        if k not in cache:
            cache[k] = pair(m.r32[k], q, strict, nudge[1] if nudge and nudge[0] == k else None)
        return cache[k]
    splits = [screen_split(hl, s * sh["kchunk"], min(K, (s + 1) * sh["kchunk"]), sh["cap"], c["kOut"], compact_drops_equal)
              for s in range(sh["nsplit"])]
    U, lost = INF32, INF32
    for s in splits:
        U, lost = np.minimum(U, s.U), np.minimum(lost, s.lost)
    if not (lost > U):
        return Result(*fb_answer(), 0, True, U, splits)
    verified, lanes = 0, []
    for sub in range(sh["L"]):
        best, bi = math.inf, 0x7fffffff
        for s in range(sub, sh["nsplit"], sh["L"]):
            for k0, l in splits[s].out:
                if l > U:
                    continue
                for k in range(k0, min(K, k0 + 8)):
                    lo = hl(k)[1]
                    if (lo >= U) if retest_strict else (lo > U):
                        continue
                    d = chi2_device(m.rec[k], p)
                    verified += 1
                    if d < best:
                        best, bi = d, k
        lanes.append((best, bi))
    best, bi = min(lanes)  # od < best || (od == best && oi < bi): chi2 of a screened point is finite
    return Result(-1 if bi == 0x7fffffff else bi, best, verified, False, U, splits)
