"""The sequential model of gl_orb_pyramid and gl_orb_detect: the irregular half of ORBextractor (orb_extractor.cpp) - ComputePyramid,
the cell FAST of ComputeKeyPointsOctTree and DistributeOctTree - restated line by line with the rules of include/gmmloc_hip.h.  Line
numbers are the reference's; nothing of it is copied.  Floats are numpy float32 / float64 scalars, one rounding per operation.  The
octree works on a real linked list (class List below), so the list order is the code's and not a derivation.
`mut`: names of rules swapped on purpose - tests/test_orb_detect_ref.py shows that each is seen by a declared case.
Test infrastructure; nothing in the product imports it."""
import math

import numpy as np

from tests.orb_ref import scale_table

f32, f64 = np.float32, np.float64
EDGE_THRESHOLD = 19  # :75
MIN_BORDER = EDGE_THRESHOLD - 3  # :747-748
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3))  # (dx, dy), radius 3, in order round the circle


def cv_round(v, mut=()):
    """cvRound: half to even (half up when swapped)"""
    if "half_up" in mut:
        return int(math.floor(float(v) + 0.5))
    return int(np.rint(v))


# ---- the pyramid
def level_sizes(width, height, nlevels, scale_factor=1.2, mut=()):
    """:1058-1060 -> [(h, w)]"""
    sf = scale_table(scale_factor)
    out = []
    for l in range(nlevels):
        inv = f32(1.0) / sf[l]  # :423
        out.append((cv_round(f32(height) * inv, mut), cv_round(f32(width) * inv, mut)))
    return out


def resize_coef(d, n_dst, n_src, mut=()):
    """-> (s, a0, a1) of destination index d"""
    scale = f64(1.0) / (f64(n_dst) / f64(n_src))
    f = f32((f64(d) + f64(0.5)) * scale - f64(0.5))
    s = int(math.floor(f))
    f = f32(f - f32(s))
    if s < 0:
        s, f = 0, f32(0.0)
    if s >= n_src - 1:
        s, f = n_src - 1, f32(0.0)
    return s, cv_round(f32(f32(1.0) - f) * f32(2048.0), mut), cv_round(f * f32(2048.0), mut)


def resize(src, shape, mut=()):
    """OpenCV's 8-bit INTER_LINEAR in fixed point as the header declares it, pixel by pixel"""
    sh, sw = src.shape
    dh, dw = shape
    cx = [resize_coef(x, dw, sw, mut) for x in range(dw)]
    cy = [resize_coef(y, dh, sh, mut) for y in range(dh)]
    S = src.astype(np.int64)
    sx = np.array([c[0] for c in cx])
    a0, a1 = np.array([c[1] for c in cx]), np.array([c[2] for c in cx])
    rows = a0 * S[:, sx] + a1 * S[:, np.minimum(sx + 1, sw - 1)]  # the row pass of every source row
    out = np.zeros((dh, dw), np.uint8)
    for y, (sy, b0, b1) in enumerate(cy):
        r0, r1 = rows[sy], rows[min(sy + 1, sh - 1)]
        if "no_shift4" in mut:
            v = (((b0 * r0) >> 20) + ((b1 * r1) >> 20) + 2) >> 2
        else:
            v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
        out[y] = v
    return out


def pyramid(image, nlevels, scale_factor=1.2, mut=()):
    """:1056-1080 without the border: each level from the one before it (:1069)"""
    levels = [np.ascontiguousarray(image)]
    for shape in level_sizes(image.shape[1], image.shape[0], nlevels, scale_factor, mut)[1:]:
        levels.append(resize(levels[-1], shape, mut))
    return levels


def features_per_level(nfeatures, nlevels, scale_factor=1.2, mut=()):
    """:429-441"""
    factor = f32(f64(1.0) / f64(scale_factor))
    desired = f32(f32(nfeatures) * f32(f32(1.0) - factor)) / f32(f32(1.0) - f32(math.pow(float(factor), float(nlevels))))
    desired = f32(desired)
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(cv_round(desired, mut))
        total += out[-1]
        desired = f32(desired * factor)
    out.append(max(nfeatures - total, 0))
    return out


# ---- cell FAST
def corner_scores(img, x0, y0, x1, y1, th, mut=()):
    """for the pixels [x0, x1) x [y0, y1) of img: the corner score where the segment test passes at th, else 0 (int array)"""
    arc = 8 if "arc8" in mut else 10 if "arc10" in mut else 9
    out = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), np.int64)
    if out.size == 0:
        return out
    I = img.astype(np.int64)
    v = I[y0:y1, x0:x1]
    d = np.stack([v - I[y0 + dy:y1 + dy, x0 + dx:x1 + dx] for dx, dy in RING])  # 16 x h x w: centre minus ring
    best = np.full(v.shape, -256, np.int64)
    passes = np.zeros(v.shape, bool)
    for k in range(16):
        a = d[[(k + j) % 16 for j in range(arc)]]
        lo, hi = a.min(0), a.max(0)  # all ring pixels darker: v - p > th; all brighter: p - v > th
        if "ge" in mut:
            passes |= (lo >= th) | (-hi >= th)
        else:
            passes |= (lo > th) | (-hi > th)
        best = np.maximum(best, np.maximum(lo, -hi))
    score = best if "score_off" in mut else best - 1  # the largest t with lo > t
    out[passes] = score[passes]
    return out


def fast_cell(img, cx0, cy0, cx1, cy1, th, mut=()):
    """cv::FAST(cell image, th, true) on the cell image [cx0, cx1) x [cy0, cy1) of the level -> [(x, y, score)] in the LEVEL's
    coordinates, rows then columns.  The region is rows [3, rows - 3), columns [3, cols - 3) of the cell image; a neighbour that is no
    corner at th or lies outside the region counts 0."""
    x0, y0, x1, y1 = cx0 + 3, cy0 + 3, cx1 - 3, cy1 - 3
    if x1 <= x0 or y1 <= y0:
        return []
    pad = 1
    if "nms_across" in mut:  # the neighbours beyond the region count what they score
        h, w = img.shape
        ex0, ey0, ex1, ey1 = max(x0 - 1, 3), max(y0 - 1, 3), min(x1 + 1, w - 3), min(y1 + 1, h - 3)
        big = corner_scores(img, ex0, ey0, ex1, ey1, th, mut)
        s = np.zeros((y1 - y0 + 2, x1 - x0 + 2), np.int64)
        s[ey0 - (y0 - 1):ey1 - (y0 - 1), ex0 - (x0 - 1):ex1 - (x0 - 1)] = big
    else:
        s = np.pad(corner_scores(img, x0, y0, x1, y1, th, mut), pad)
    keys = []
    for ry, rx in zip(*np.nonzero(s[1:-1, 1:-1])):
        c = s[ry + 1, rx + 1]
        nb = [s[ry + 1 + dy, rx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
        if all(c >= n for n in nb) if "nonstrict" in mut else all(c > n for n in nb):
            keys.append((x0 + int(rx), y0 + int(ry), int(c)))
    return keys


def cells(width, height):
    """the cell grid of a level (:747-778) -> (nCols, nRows, [(i, j, iniX, iniY, maxX, maxY)]) without the cells the two `continue`s skip"""
    min_bx = min_by = MIN_BORDER
    max_bx, max_by = width - EDGE_THRESHOLD + 3, height - EDGE_THRESHOLD + 3
    W = f32(30)
    fw, fh = f32(max_bx - min_bx), f32(max_by - min_by)
    n_cols, n_rows = int(fw / W), int(fh / W)
    if n_cols < 1 or n_rows < 1:  # deviation 1
        return n_cols, n_rows, []
    w_cell, h_cell = int(math.ceil(fw / f32(n_cols))), int(math.ceil(fh / f32(n_rows)))
    out = []
    for i in range(n_rows):
        ini_y = min_by + i * h_cell
        max_y = ini_y + h_cell + 6
        if ini_y >= max_by - 3:  # :767
            continue
        max_y = min(max_y, max_by)
        for j in range(n_cols):
            ini_x = min_bx + j * w_cell
            max_x = ini_x + w_cell + 6
            if ini_x >= max_bx - 6:  # :775
                continue
            max_x = min(max_x, max_bx)
            out.append((i, j, ini_x, ini_y, max_x, max_y))
    return n_cols, n_rows, out


def candidates(img, ini_th=20, min_th=7, mut=()):
    """vToDistributeKeys of a level (:763-799) -> ([(x, y, score)] in ROI coordinates, cells redone at min_th)"""
    h, w = img.shape
    grid = cells(w, h)[2]
    per_cell = [fast_cell(img, x0, y0, x1, y1, ini_th, mut) for _, _, x0, y0, x1, y1 in grid]
    redo = [not k for k in per_cell]
    if "level_fallback" in mut:
        redo = [all(redo)] * len(grid)
    keys, fell = [], 0
    for (_, _, x0, y0, x1, y1), k, r in zip(grid, per_cell, redo):
        if r:  # :785-788
            fell += 1
            k = fast_cell(img, x0, y0, x1, y1, min_th, mut)
        keys.extend(k)
    return keys, fell


# ---- the octree
class Node:
    def __init__(self, x0, x1, y0, y1):
        self.x0, self.x1, self.y0, self.y1 = x0, x1, y0, y1  # UL.x, UR.x, UL.y, BL.y
        self.keys, self.no_more = [], False
        self.prev = self.next = None  # the list's links
        self.born = -1  # creation order, for the declared tie of phase 2

    def divide(self, mut=()):
        """DivideNode (:475-527)"""
        up = math.floor if "floor_half" in mut else math.ceil
        half_x, half_y = int(up(f32(self.x1 - self.x0) / f32(2))), int(up(f32(self.y1 - self.y0) / f32(2)))
        mx, my = self.x0 + half_x, self.y0 + half_y
        n = [Node(self.x0, mx, self.y0, my), Node(mx, self.x1, self.y0, my), Node(self.x0, mx, my, self.y1), Node(mx, self.x1, my, self.y1)]
        for k in self.keys:
            if k[0] < mx:
                n[0 if k[1] < my else 2].keys.append(k)
            else:
                n[1 if k[1] < my else 3].keys.append(k)
        for c in n:
            c.no_more = len(c.keys) == 1
        return n


class List:
    """std::list<ExtractorNode>: doubly linked, push_front / push_back / erase"""

    def __init__(self):
        self.head = self.tail = None
        self.size = 0

    def push_front(self, n):
        n.prev, n.next = None, self.head
        if self.head:
            self.head.prev = n
        self.head = n
        self.tail = self.tail or n
        self.size += 1

    def push_back(self, n):
        n.prev, n.next = self.tail, None
        if self.tail:
            self.tail.next = n
        self.tail = n
        self.head = self.head or n
        self.size += 1

    def erase(self, n):
        """-> the node behind it"""
        if n.prev:
            n.prev.next = n.next
        else:
            self.head = n.next
        if n.next:
            n.next.prev = n.prev
        else:
            self.tail = n.prev
        self.size -= 1
        return n.next

    def __iter__(self):
        n = self.head
        while n:
            yield n
            n = n.next


def nth_permutation(k, n):
    """the k-th permutation of range(n) in lexicographic order (0: the identity)"""
    items, out = list(range(n)), []
    for i in range(n, 0, -1):
        q, k = divmod(k, math.factorial(i - 1))
        out.append(items.pop(q))
    return out


def distribute(keys, min_x, max_x, min_y, max_y, N, mut=(), info=None, tie_order=None):
    """DistributeOctTree (:529-737).  keys: [(x, y, response)] relative to (min_x, min_y), in vToDistributeKeys' order -> vResultKeys
    info: a dict that is filled with what happened -
      tie         a phase-2 sort (:664) saw two entries of equal size: the reference's order there is the allocator's (deviation 4)
      sorts       the phase-2 sorts that held two or more entries
      walked      the most nodes that one phase-2 pass divided
      end         "sweep N" (:649, size >= N), "sweep same" (:649, size == prevSize), "phase 2 N" / "phase 2 same" (:710)
      sweeps      the sweeps of phase 1 that ran
      phase1      the list's size when phase 1 ended: no result is shorter, whatever the order among equal sizes
      n_ini       nIni
      groups      the sizes of the equal-size groups of two or more that phase 2 REACHED, in the order it reached them
    tie_order: None - the declared order among equal sizes; else a list of choices, one per reached group in that order: the group is
      walked in the choice-th permutation (lexicographic) of its declared order; groups beyond the list take choice 0"""
    if info is None:
        info = {}
    info.update(tie=False, sorts=0, walked=0, end=None, sweeps=0, phase1=0, n_ini=0, groups=[])
    n_ini = int(math.floor(float(f32(max_x - min_x) / f32(max_y - min_y)) + 0.5))  # :535, round() of a positive float
    info["n_ini"] = n_ini
    if n_ini < 1:  # deviation 2
        return []
    h_x = f32(max_x - min_x) / f32(n_ini)
    nodes, born = List(), [0]
    push = nodes.push_back if "push_back" in mut else nodes.push_front

    def add(n, to_expand):
        n.born = born[0]
        born[0] += 1
        push(n)
        if len(n.keys) > 1:
            to_expand.append(n)

    ini = []
    for i in range(n_ini):
        if "rational_edge" in mut:  # the edges as exact fractions instead of the float products of :546-547
            n = Node((max_x - min_x) * i // n_ini, (max_x - min_x) * (i + 1) // n_ini, 0, max_y - min_y)
        else:
            n = Node(int(h_x * f32(i)), int(h_x * f32(i + 1)), 0, max_y - min_y)
        nodes.push_back(n)
        ini.append(n)
    for k in keys:
        ini[min(int(f32(k[0]) / h_x), n_ini - 1)].keys.append(k)  # :559, deviation 3
    n = nodes.head
    while n:  # :564-572
        if len(n.keys) == 1:
            n.no_more = True
            n = n.next
        elif not n.keys:
            n = nodes.erase(n)
        else:
            n = n.next
    finish = False
    to_expand = []
    while not finish:
        prev_size = nodes.size
        to_expand = []
        n_to_expand = 0
        n = nodes.head
        while n:  # :594-645
            if n.no_more:
                n = n.next
                continue
            before = len(to_expand)
            for c in n.divide(mut):
                if c.keys:
                    add(c, to_expand)
            n_to_expand += len(to_expand) - before
            n = nodes.erase(n)
        info["sweeps"] += 1
        info["phase1"] = nodes.size
        if nodes.size >= N or nodes.size == prev_size:  # :649
            finish = True
            info["end"] = "sweep N" if nodes.size >= N else "sweep same"
        elif nodes.size + n_to_expand * 3 > N:  # :653
            while not finish:
                prev_size = nodes.size
                prev, to_expand = to_expand, []
                # :664 sorts (size, pointer) and walks from the back.  Deviation 4: among equal sizes the node created last goes first
                prev.sort(key=lambda n: (len(n.keys), -n.born if "tie_rev" in mut else n.born))
                sizes = [len(n.keys) for n in prev]
                info["sorts"] += len(prev) >= 2
                info["tie"] = info["tie"] or len(set(sizes)) < len(sizes)
                walk, walked = prev[::-1], 0
                i = 0
                while i < len(walk):
                    j = i
                    while j < len(walk) and len(walk[j].keys) == len(walk[i].keys):
                        j += 1
                    if j - i > 1:  # a group of equal sizes is reached: its order is the caller's choice, the declared one by default
                        at = len(info["groups"])
                        info["groups"].append(j - i)
                        if tie_order is not None and at < len(tie_order):
                            walk[i:j] = [walk[i + q] for q in nth_permutation(tie_order[at], j - i)]
                    stop = False
                    for n in walk[i:j]:
                        walked += 1
                        for c in n.divide(mut):
                            if c.keys:
                                add(c, to_expand)
                        nodes.erase(n)
                        if nodes.size >= N:  # :706
                            stop = True
                            break
                    if stop:
                        break
                    i = j
                info["walked"] = max(info["walked"], walked)
                if nodes.size >= N or nodes.size == prev_size:  # :710
                    finish = True
                    info["end"] = "phase 2 N" if nodes.size >= N else "phase 2 same"
    out = []
    for n in nodes:  # :720-734
        best = n.keys[0]
        for k in n.keys[1:]:
            if k[2] > best[2]:
                best = k
        out.append(best)
    return out


def level_bound(width, height, n_level):
    """the most key-points a level can yield: max(N_l + 2, 4 nIni_l); 0 for a level of deviation 1 or 2"""
    w, h = width - 2 * MIN_BORDER, height - 2 * MIN_BORDER
    if w < 30 or h < 30:
        return 0
    n_ini = int(math.floor(float(f32(w) / f32(h)) + 0.5))
    return max(n_level + 2, 4 * n_ini) if n_ini >= 1 else 0


def detect(levels, nfeatures, scale_factor=1.2, ini_th=20, min_th=7, cand_cap=None, mut=()):
    """gl_orb_detect for ONE image: levels - its pyramid, 2-D uint8 arrays.  -> dict(kp_xy n x 2, kp_oct n, kp_response n, level_count 8,
    stat 4, cand [per level: m x 3 (x, y, score)], cand_count 8, tie [per level: a phase-2 sort saw two equal sizes, so the reference's
    order on that level is its allocator's], sorts [per level: the phase-2 sorts of two or more entries])"""
    per_level = features_per_level(nfeatures, len(levels), scale_factor, mut)
    xy, octs, resp, level_count, cand, fell, mask = [], [], [], [0] * 8, [], 0, 0
    tie, sorts = [False] * len(levels), [0] * len(levels)
    for l, img in enumerate(levels):
        h, w = img.shape
        keys, f = candidates(img, ini_th, min_th, mut)
        fell += f
        cand.append(np.array(keys, np.int32).reshape(-1, 3))
        if cand_cap is not None and len(keys) > cand_cap:  # deviation 5
            mask |= 1 << l
            continue
        rel = [(x - MIN_BORDER, y - MIN_BORDER, s) for x, y, s in keys]
        info = {}
        res = distribute(rel, MIN_BORDER, w - MIN_BORDER, MIN_BORDER, h - MIN_BORDER, per_level[l], mut, info) if keys else []
        tie[l], sorts[l] = bool(info.get("tie")), int(info.get("sorts", 0))
        for x, y, s in res:  # :813-816
            xy.append((x + MIN_BORDER, y + MIN_BORDER))
            octs.append(l)
            resp.append(s)
        level_count[l] = len(res)
    if mask:
        xy, octs, resp, level_count = [], [], [], [0] * 8
    cand_count = [len(c) for c in cand] + [0] * (8 - len(cand))
    return dict(kp_xy=np.array(xy, np.int32).reshape(-1, 2), kp_oct=np.array(octs, np.int32), kp_response=np.array(resp, np.float32),
                level_count=np.array(level_count, np.int32), stat=np.array([sum(cand_count), fell, len(octs), mask], np.int32), cand=cand,
                cand_count=np.array(cand_count, np.int32), tie=tie, sorts=sorts)
