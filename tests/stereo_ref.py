"""Frame::computeStereoMatches (frame.cpp:179-349) restated as a SEQUENTIAL model in numpy - the reference side of every comparison of
gl_stereo_matches (tests/test_stereo_ref.py, tests/test_gpu_stereo*.py).  Test infrastructure; nothing in the product imports it.

It follows the reference statement by statement, the lines cited at each; every float operation is an explicit np.float32 (one rounding
per operation), every double operation an np.float64.  It carries the five declared deviations of include/gmmloc_hip.h - each a place
where the reference indexes out of range or throws - marked `deviation n` where they act.  The reference binary needs OpenCV, which the
test machines lack, so parity with it stays unpinned: this file is a restatement, not a recording.

`mut`: a set of rule names, each of which swaps ONE decision for its neighbour (a float product for a double one, `<` for `<=`, ...).
The device never sees them; tests/test_stereo_ref.py uses them to show that the hand-built cases can see every rule."""
import numpy as np

f32, f64 = np.float32, np.float64
TH_HIGH, TH_LOW = 100, 50  # ORBmatcher::TH_HIGH / TH_LOW (orb_matcher.h)
MUTATIONS = ("band_lo_strict", "band_hi_strict", "band_double", "row_rounded", "oct_lo_strict", "oct_hi_strict", "minu_strict", "maxu_strict",
             "maxu_skip_le", "init_le", "desc_le", "th_le", "ul_float_product", "ur_double_product", "round_half_even", "endu_gt",
             "sad_le", "edge_keep", "delta_double", "disp_gt", "disp_le_maxd", "zero_branch_float", "median_low", "th_gt", "th_double")


def scale_tables(scale_factor, n=8):
    """frame::scale_factors / scale_factors_inv (init_config.hpp:63-79): float, repeated multiply"""
    sf, inv = [f32(1.0)], [f32(1.0)]
    for _ in range(1, n):
        sf.append(f32(sf[-1] * f32(scale_factor)))
        inv.append(f32(f32(1.0) / sf[-1]))
    return np.array(sf, f32), np.array(inv, f32)


def c_round(x):
    """round(): half away from zero, in x's own format (|x| - floor(|x|) is exact)"""
    a = np.abs(x)
    r = np.floor(a)
    if a - r >= 0.5:
        r = r + type(x)(1)
    return type(x)(np.copysign(r, x))


def hamming(a, b):
    """ORBmatcher::DescriptorDistance (orb_matcher.cpp:580-596)"""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def stereo_matches(cam, scale_factor, feat_uv, feat_oct, feat_desc, r_uv, r_oct, r_desc, pyr_left, pyr_right, n_left=None, n_right=None,
                   mut=()):
    """ONE frame.  cam: (fx, bf, height).  feat_uv (NF, 2) f64, feat_oct (NF,), feat_desc (NF, 32) u8; r_uv (NR, 2) f32, r_oct, r_desc;
    pyr_left / pyr_right: the level images (2-D u8 arrays, the ROI).  -> dict: feat_ur, feat_depth (NF,) f32, match_r, sad (NF,) i32,
    stat (4,) i32, and `dropped`: {line: count} of the features that left at :261, :287, :306, :316, :325."""
    assert all(m in MUTATIONS for m in mut), mut
    fx, bf, height = cam
    nlevels = len(pyr_left)
    sf, sf_inv = scale_tables(scale_factor)
    NF, NR = len(feat_oct), len(r_oct)
    nL = NF if n_left is None else min(max(int(n_left), 0), NF)
    nR = NR if n_right is None else min(max(int(n_right), 0), NR)
    th_desc_dist = (TH_HIGH + TH_LOW) // 2                                       # :183
    nRows = int(height)                                                          # :185
    vRowIndices = [[] for _ in range(nRows)]                                     # :188
    for iR in range(nR):                                                         # :195
        octave = int(r_oct[iR])
        if octave < 0 or octave >= nlevels:                                      # deviation 3
            continue
        kpY = f32(r_uv[iR, 1])                                                   # :197
        if "band_double" in mut:
            r = f64(2.0) * f64(sf[octave])
            maxr, minr = np.ceil(f64(kpY) + r), np.floor(f64(kpY) - r)
        else:
            r = f32(f32(2.0) * sf[octave])                                       # :198
            maxr, minr = np.ceil(f32(kpY + r)), np.floor(f32(kpY - r))           # :199-200
        if not (maxr >= 0 and minr < nRows):                                     # (no row inside the image; NaN)
            continue
        lo = int(minr) + ("band_lo_strict" in mut)
        hi = int(maxr) - ("band_hi_strict" in mut)
        for yi in range(max(lo, 0), min(hi, nRows - 1) + 1):                     # :202, deviation 1
            vRowIndices[yi].append(iR)                                           # :203
    mbf = f32(bf)                                                                # frame.cpp:23
    mb = f32(f64(bf) / f64(fx))                                                  # frame.cpp:24
    minZ, minD = mb, f32(0.0)                                                    # :208-209
    maxD = f32(mbf / minZ)                                                       # :210
    ur = np.full(NF, -1.0, f32)
    depth = np.full(NF, -1.0, f32)
    match_r = np.full(NF, -1, np.int32)
    sad = np.full(NF, -1, np.int32)
    dropped = {261: 0, 287: 0, 306: 0, 316: 0, 325: 0}
    n261 = 0
    vDistIdx = []                                                                # :213
    for iL in range(nL):                                                         # :217
        levelL = int(feat_oct[iL])                                               # :219
        if levelL < 0 or levelL >= nlevels:                                      # deviation 3
            continue
        vL, uL = f32(feat_uv[iL, 1]), f32(feat_uv[iL, 0])                        # :220-221
        if not (vL >= 0 and vL < nRows):                                         # deviation 2
            continue
        row = int(c_round(vL)) if "row_rounded" in mut else int(vL)              # :223, (size_t)vL truncates
        if row >= nRows:
            continue
        vCandidates = vRowIndices[row]
        if not vCandidates:                                                      # :225
            continue
        minU, maxU = f32(uL - maxD), f32(uL - minD)                              # :228-229
        if (maxU <= 0) if "maxu_skip_le" in mut else (maxU < 0):                 # :231
            continue
        bestDist, bestIdxR = TH_HIGH + ("init_le" in mut), 0                     # :234-235
        for iR in vCandidates:                                                   # :240
            octave = int(r_oct[iR])
            if octave < levelL - 1 + ("oct_lo_strict" in mut) or octave > levelL + 1 - ("oct_hi_strict" in mut):  # :244
                continue
            uR = f32(r_uv[iR, 0])                                                # :247
            ok_lo = uR > minU if "minu_strict" in mut else uR >= minU
            ok_hi = uR < maxU if "maxu_strict" in mut else uR <= maxU
            if ok_lo and ok_hi:                                                  # :249
                dist = hamming(feat_desc[iL], r_desc[iR])                        # :251
                if (dist <= bestDist) if "desc_le" in mut else (dist < bestDist):  # :253
                    bestDist, bestIdxR = dist, iR
        if not ((bestDist <= th_desc_dist) if "th_le" in mut else (bestDist < th_desc_dist)):  # :261
            dropped[261] += 1
            continue
        n261 += 1
        uR0 = f32(r_uv[bestIdxR, 0])                                             # :263
        scaleFactor = sf_inv[levelL]                                             # :264
        rnd = (lambda x: type(x)(np.rint(x))) if "round_half_even" in mut else c_round
        if "ul_float_product" in mut:
            scaleduL = f32(rnd(f32(f32(feat_uv[iL, 0]) * scaleFactor)))
            scaledvL = f32(rnd(f32(f32(feat_uv[iL, 1]) * scaleFactor)))
        else:
            scaleduL = f32(rnd(f64(feat_uv[iL, 0]) * f64(scaleFactor)))          # :265, a double product
            scaledvL = f32(rnd(f64(feat_uv[iL, 1]) * f64(scaleFactor)))          # :266
        if "ur_double_product" in mut:
            scaleduR0 = f32(rnd(f64(uR0) * f64(scaleFactor)))
        else:
            scaleduR0 = f32(rnd(f32(uR0 * scaleFactor)))                         # :267, a float product
        w, L = 5, 5                                                              # :270, :279
        IL_img, IR_img = pyr_left[levelL], pyr_right[levelL]
        iniu = f32(f32(scaleduR0 + f32(L)) - f32(w))                             # :284
        endu = f32(f32(f32(scaleduR0 + f32(L)) + f32(w)) + f32(1))               # :285
        cols = IR_img.shape[1]
        if iniu < 0 or ((endu > cols) if "endu_gt" in mut else (endu >= cols)):  # :286
            dropped[287] += 1
            continue
        inside = (scaledvL - w >= 0 and scaledvL + w < min(IL_img.shape[0], IR_img.shape[0]) and scaleduL - w >= 0 and
                  scaleduL + w < IL_img.shape[1] and scaleduR0 - L - w >= 0 and scaleduR0 + L + w < cols)
        if not inside:                                                           # deviation 4 (rowRange / colRange throw)
            dropped[287] += 1
            continue
        cu, cv, cr = int(scaleduL), int(scaledvL), int(scaleduR0)
        IL = IL_img[cv - w:cv + w + 1, cu - w:cu + w + 1].astype(np.int64)       # :271-274
        IL = IL - IL[w, w]                                                       # :275
        bestSAD, bestincR = None, 0                                              # :277-278 (INT_MAX)
        vDists = [0] * (2 * L + 1)                                               # :281
        for incR in range(-L, L + 1):                                            # :289
            IR = IR_img[cv - w:cv + w + 1, cr + incR - w:cr + incR + w + 1].astype(np.int64)  # :290-294
            IR = IR - IR[w, w]                                                   # :295
            dist = int(np.abs(IL - IR).sum())                                    # :297, integers: exact in float
            if bestSAD is None or ((dist <= bestSAD) if "sad_le" in mut else (dist < bestSAD)):  # :298
                bestSAD, bestincR = dist, incR
            vDists[L + incR] = dist                                              # :303
        if (bestincR == -L or bestincR == L) and "edge_keep" not in mut:         # :306
            dropped[306] += 1
            continue
        if bestincR == -L or bestincR == L:  # (edge_keep: the missing neighbour taken as the best itself)
            vDists = [vDists[0]] + vDists + [vDists[-1]]
            base = 1
        else:
            base = 0
        dist1 = f32(vDists[base + L + bestincR - 1])                             # :309
        dist2 = f32(vDists[base + L + bestincR])                                 # :310
        dist3 = f32(vDists[base + L + bestincR + 1])                             # :311
        den = f32(f32(2.0) * f32(f32(dist1 + dist3) - f32(f32(2.0) * dist2)))
        with np.errstate(divide="ignore", invalid="ignore"):
            if "delta_double" in mut:
                deltaR = f64(f64(dist1) - f64(dist3)) / f64(den)
            else:
                deltaR = f32(f32(dist1 - dist3) / den)                           # :313-314
        if deltaR < -1 or deltaR > 1:                                            # :316
            dropped[316] += 1
            continue
        bestuR = f32(sf[levelL] * f32(f32(f32(scaleduR0) + f32(bestincR)) + f32(deltaR)))  # :320-321
        disparity = f32(uL - bestuR)                                             # :323
        ok_lo = disparity > minD if "disp_gt" in mut else disparity >= minD
        ok_hi = disparity <= maxD if "disp_le_maxd" in mut else disparity < maxD
        if not (ok_lo and ok_hi):                                                # :325
            dropped[325] += 1
            continue
        if disparity <= 0:                                                       # :326
            disparity = f32(0.01)                                                # :327
            bestuR = f32(uL - f32(0.01)) if "zero_branch_float" in mut else f32(f64(uL) - f64(0.01))  # :328
        depth[iL] = f32(mbf / disparity)                                         # :330
        ur[iL] = bestuR                                                          # :331
        match_r[iL], sad[iL] = bestIdxR, bestSAD
        vDistIdx.append((bestSAD, iL))                                           # :332
    median, nreset = -1, 0
    if vDistIdx:                                                                 # deviation 5
        vDistIdx.sort()                                                          # :337
        pos = (len(vDistIdx) - 1) // 2 if "median_low" in mut else len(vDistIdx) // 2
        median = vDistIdx[pos][0]                                                # :338
        if "th_double" in mut:
            thDist = f64(1.5) * f64(1.4) * f64(median)
        else:
            thDist = f32(f32(f32(1.5) * f32(1.4)) * f32(median))                 # :339
        for s, iL in reversed(vDistIdx):                                         # :341
            if (f32(s) <= thDist) if "th_gt" in mut else (f32(s) < thDist):      # :342
                break
            depth[iL] = f32(-1.0)                                                # :345
            ur[iL] = f32(-1.0)                                                   # :346
            nreset += 1
    return {"feat_ur": ur, "feat_depth": depth, "match_r": match_r, "sad": sad,
            "stat": np.array([n261, len(vDistIdx), nreset, median], np.int32), "dropped": dropped}


def stereo_matches_batch(cam, scale_factor, frames):
    """`frames`: a list of dicts with the keyword arguments of stereo_matches -> the outputs stacked (the frames share NF)"""
    outs = [stereo_matches(cam, scale_factor, **f) for f in frames]
    return {k: np.stack([o[k] for o in outs]) for k in ("feat_ur", "feat_depth", "match_r", "sad", "stat")}
