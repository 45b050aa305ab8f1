"""The covisibility graph and the two lists of searchInNeighbors said twice, the checker of tests/test_covis_ref.py, tests/
test_gpu_covis_cases.py and tests/test_gpu_covis.py (gl_covis_update, gl_covis_remove, gl_covis_best, gl_fuse_targets,
gl_fuse_candidates).  Test infrastructure; nothing in the product imports it.

Model   a sequential OBJECT model: per key-frame a dict for map_frame_weights_ and lists for ordered_keyframes_ / ordered_weights_,
        with addConnection, updateBestCovisibles, updateConnections, removeConnection, the graph part of Map::removeKeyFrame, the target
        loop and the candidate loop restated statement for statement (keyframe.cpp:116-150, :243-330, map.cpp:60-87, localization.cpp:
        155-206).  Only the DECLARED orders stand in for pointer and hash order: ties of weight go to the lowest row, the target set is
        iterated in insertion order, and an empty ordered list at map.cpp:82 leaves best_cov_kf_ alone and is reported.
Rows    the ROW REPRESENTATION the device keeps (sorted rows cov_kf / cov_w, cov_n, the prefix length cov_nord, best_cov), each call
        stated on the arrays with numpy - with the capacity rule and the handling of malformed rows, which the object model has no
        notion of.
A map is a dict of numpy arrays: kf_mp (NKF,NFK), mp_valid (NMP,), obs_ptr (NMP+1,), obs_kf (NOBS,), kf_valid (NKF,)."""
import numpy as np

TH = 15  # keyframe.cpp:280
KEPT, TRUNCATED, BAD_ROW = 1, 2, 4
W_TRUNCATED, EMPTY_LIST, COVIS_BAD_ROW, LIST_TRUNCATED = 8, 16, 32, 64
SENTINEL = -77


def counter(m, kf):
    """KFcounter of key-frame row kf (keyframe.cpp:253-272) as {row: count}, rows outside the table and malformed CSR ranges skipped as
    gl_update_connections skips them"""
    NMP, NKF, NOBS = len(m["obs_ptr"]) - 1, m["kf_mp"].shape[0], len(m["obs_kf"])
    c = {}
    for p in m["kf_mp"][kf].tolist():
        if p < 0 or p >= NMP or not m["mp_valid"][p]:  # (:257-261)
            continue
        a, b = int(m["obs_ptr"][p]), int(m["obs_ptr"][p + 1])
        if not (0 <= a <= b <= NOBS):
            continue
        for k in m["obs_kf"][a:b].tolist():
            if k < 0 or k >= NKF or k == kf:  # (:268-269)
                continue
            c[k] = c.get(k, 0) + 1
    return c


def declared(pairs):
    """(row, weight) pairs in the declared order: weight descending, ties to the lowest row"""
    return sorted(pairs, key=lambda kw: (-kw[1], kw[0]))


class KeyFrame:
    def __init__(self, row):
        self.row = row
        self.weights = {}   # map_frame_weights_
        self.ordered = []   # ordered_keyframes_
        self.ordered_w = []  # ordered_weights_
        self.best = -1      # best_cov_kf_


class Model:
    def __init__(self, NKF):
        self.kfs = [KeyFrame(r) for r in range(NKF)]

    # keyframe.cpp:116-128
    def add_connection(self, kf, other, weight):
        k = self.kfs[kf]
        if other not in k.weights:
            k.weights[other] = weight
        elif k.weights[other] != weight:
            k.weights[other] = weight
        else:
            return
        self.update_best_covisibles(kf)

    # keyframe.cpp:130-150: the WHOLE weight map, entries below 15 included
    def update_best_covisibles(self, kf):
        k = self.kfs[kf]
        pairs = declared(k.weights.items())
        k.ordered = [r for r, _ in pairs]
        k.ordered_w = [w for _, w in pairs]

    # keyframe.cpp:243-316 -> status
    def update_connections(self, m, kf):
        c = counter(m, kf)
        if not c:  # (:275-276)
            return KEPT
        nmax, kfmax = 0, None
        pairs = []
        for r in sorted(c):  # (the declared stand-in for the unordered_map's order: the largest at the lowest row)
            if c[r] > nmax:
                nmax, kfmax = c[r], r
            if c[r] >= TH:
                pairs.append((r, c[r]))
                self.add_connection(r, kf, c[r])
        if not pairs:
            pairs.append((kfmax, nmax))
            self.add_connection(kfmax, kf, nmax)
        pairs = declared(pairs)
        k = self.kfs[kf]
        k.weights = dict(c)
        k.ordered = [r for r, _ in pairs]
        k.ordered_w = [w for _, w in pairs]
        return 0

    # keyframe.cpp:318-330
    def remove_connection(self, kf, other):
        k = self.kfs[kf]
        if other in k.weights:
            del k.weights[other]
            self.update_best_covisibles(kf)
            return True
        return False

    # map.cpp:60-87, the graph part -> (removed, erased entries, status)
    def remove_key_frame(self, r, kf_first):
        if r == kf_first:  # (:63)
            return 0, 0, 0
        k = self.kfs[r]
        erased = sum(self.remove_connection(o, r) for o in list(k.weights) if o != r)
        status = 0
        if k.ordered:
            k.best = k.ordered[0]  # (:82)
        else:
            status = EMPTY_LIST  # declared: the reference indexes an empty vector
        k.weights = {}
        k.ordered, k.ordered_w = [], []
        return 1, erased, status

    def best_covisibles(self, kf, N):  # keyframe.cpp:163-170, N <= 0: :152-155
        k = self.kfs[kf]
        n = len(k.ordered) if N <= 0 else min(N, len(k.ordered))
        return k.ordered[:n], k.ordered_w[:n]

    # localization.cpp:155-179 -> the targets in insertion order
    def fuse_targets(self, kf_row, kf_valid, nn=10, nn2=5):
        tgt = []
        for kf1 in self.best_covisibles(kf_row, nn)[0] if nn > 0 else []:
            if not kf_valid[kf1] or kf1 in tgt:
                continue
            tgt.append(kf1)
            for kf2 in self.best_covisibles(kf1, nn2)[0] if nn2 > 0 else []:
                if not kf_valid[kf2] or kf2 in tgt or kf2 == kf_row:
                    continue
                tgt.append(kf2)
        return tgt

    def rows(self, Wcap, fill=SENTINEL):
        """-> the row representation; asserts what it rests on: the ordered list is a prefix of the row in the declared order"""
        NKF = len(self.kfs)
        out = dict(cov_kf=np.full((NKF, Wcap), fill, np.int32), cov_w=np.full((NKF, Wcap), fill, np.int32), cov_n=np.zeros(NKF, np.int32),
                   cov_nord=np.zeros(NKF, np.int32), best_cov=np.zeros(NKF, np.int32))
        for k in self.kfs:
            pairs = declared(k.weights.items())
            n, nord = len(pairs), len(k.ordered)
            assert n <= Wcap, (k.row, n, Wcap)
            assert list(zip(k.ordered, k.ordered_w)) == pairs[:nord], (k.row, k.ordered, k.ordered_w, pairs)
            out["cov_kf"][k.row, :n] = [r for r, _ in pairs]
            out["cov_w"][k.row, :n] = [w for _, w in pairs]
            out["cov_n"][k.row], out["cov_nord"][k.row], out["best_cov"][k.row] = n, nord, k.best
        return out

    @staticmethod
    def from_rows(g):
        """the model of a WELL-FORMED row representation (distinct in-table entries, sorted rows)"""
        md = Model(len(g["cov_n"]))
        for k in md.kfs:
            n, nord = int(g["cov_n"][k.row]), int(g["cov_nord"][k.row])
            k.weights = dict(zip(g["cov_kf"][k.row, :n].tolist(), g["cov_w"][k.row, :n].tolist()))
            k.ordered, k.ordered_w = g["cov_kf"][k.row, :nord].tolist(), g["cov_w"][k.row, :nord].tolist()
            k.best = int(g["best_cov"][k.row])
        return md


# localization.cpp:188-206 -> the candidates in walk order
def fuse_candidates(m, targets, kf_idx):
    NMP, NKF = len(m["mp_valid"]), m["kf_mp"].shape[0]
    stamp = np.zeros(NMP, np.int64)  # fuse_tgt_kf_ = 0 (mappoint.h:95)
    out = []
    for kf in targets:
        if kf < 0 or kf >= NKF:
            continue
        for p in m["kf_mp"][kf].tolist():
            if p < 0 or p >= NMP or not m["mp_valid"][p] or stamp[p] == kf_idx:
                continue
            stamp[p] = kf_idx
            out.append(p)
    return out


# ---------------------------------------------------------------------------------------------------- the row representation, in numpy
def _len(g, k):
    return int(np.clip(g["cov_n"][k], 0, g["cov_kf"].shape[1]))


def _ord(g, k):
    return int(np.clip(g["cov_nord"][k], 0, _len(g, k)))


def _sorted(kf, w):
    o = np.lexsort((kf, -w.astype(np.int64)))
    return kf[o], w[o]


def rows_update(g, m, kf, Ccap):
    """gl_covis_update on the arrays IN PLACE -> dict(conn_kf, conn_w (Ccap,), n_conn, result (4,)); conn_* entries beyond the list: 0"""
    W = g["cov_kf"].shape[1]
    c = counter(m, kf)
    out = dict(conn_kf=np.zeros(Ccap, np.int32), conn_w=np.zeros(Ccap, np.int32), n_conn=np.zeros(1, np.int32), result=np.zeros(4, np.int32))
    if not c:
        out["result"][1] = KEPT
        return out
    rk, rw = _sorted(np.array(list(c), np.int32), np.array(list(c.values()), np.int32))
    nord = max(int((rw >= TH).sum()), 1)
    n = min(nord, Ccap)
    out["conn_kf"][:n], out["conn_w"][:n], out["n_conn"][0] = rk[:n], rw[:n], nord
    status = TRUNCATED if nord > Ccap else 0
    widest = len(rk)
    for k in rk[:nord].tolist():
        widest = max(widest, _len(g, k) + (0 if kf in g["cov_kf"][k, :_len(g, k)] else 1))
    out["result"][:2] = widest, status | (W_TRUNCATED if widest > W else 0)
    if widest > W:
        return out
    g["cov_kf"][kf, :len(rk)], g["cov_w"][kf, :len(rk)], g["cov_n"][kf], g["cov_nord"][kf] = rk, rw, len(rk), nord
    for k, w in zip(rk[:nord].tolist(), rw[:nord].tolist()):
        n = _len(g, k)
        a, b = g["cov_kf"][k, :n].copy(), g["cov_w"][k, :n].copy()
        hit = np.flatnonzero(a == kf)
        if len(hit) and b[hit[0]] == w:
            continue
        if len(hit):
            a, b = np.delete(a, hit[0]), np.delete(b, hit[0])
        at = int(((b > w) | ((b == w) & (a < kf))).sum())  # the entries the declared order puts in front of (kf, w)
        a, b = np.insert(a, at, kf), np.insert(b, at, w)
        g["cov_kf"][k, :len(a)], g["cov_w"][k, :len(a)] = a, b
        g["cov_n"][k] = g["cov_nord"][k] = len(a)
        out["result"][2] += 1
    return out


def rows_remove(g, NKF, rows, kf_first):
    """gl_covis_remove on the arrays IN PLACE -> result (4,)"""
    removed = erased = bad = status = 0
    for r in rows:
        if r < 0 or r >= NKF:
            bad += 1
            continue
        if r == kf_first:
            continue
        named = g["cov_kf"][r, :_len(g, r)].tolist()
        for j, k in enumerate(named):
            if k < 0 or k >= NKF:
                bad += 1
                continue
            if k == r or k in named[:j]:
                continue
            n = _len(g, k)
            hit = np.flatnonzero(g["cov_kf"][k, :n] == r)
            if not len(hit):
                continue
            for a in ("cov_kf", "cov_w"):
                g[a][k, hit[0]:n - 1] = g[a][k, hit[0] + 1:n].copy()
            g["cov_n"][k] = g["cov_nord"][k] = n - 1
            erased += 1
        if _ord(g, r) > 0:
            g["best_cov"][r] = g["cov_kf"][r, 0]
        else:
            status |= EMPTY_LIST
        g["cov_n"][r] = g["cov_nord"][r] = 0
        removed += 1
    return np.array([removed, status | (COVIS_BAD_ROW if bad else 0), erased, bad], np.int32)


def rows_best(g, NKF, kf_rows, N, Ccap):
    """gl_covis_best -> dict(conn_kf, conn_w (B,Ccap), n_conn (B,), result (4,)); entries beyond a list: 0"""
    B = len(kf_rows)
    out = dict(conn_kf=np.zeros((B, Ccap), np.int32), conn_w=np.zeros((B, Ccap), np.int32), n_conn=np.zeros(B, np.int32), result=np.zeros(4, np.int32))
    for b, k in enumerate(kf_rows):
        if k < 0 or k >= NKF:
            out["result"][1] |= COVIS_BAD_ROW
            out["result"][3] += 1
            continue
        n = _ord(g, k) if N <= 0 else min(N, _ord(g, k))
        out["conn_kf"][b, :min(n, Ccap)], out["conn_w"][b, :min(n, Ccap)] = g["cov_kf"][k, :min(n, Ccap)], g["cov_w"][k, :min(n, Ccap)]
        out["n_conn"][b] = n
        if n > Ccap:
            out["result"][1] |= TRUNCATED
    return out


def rows_targets(g, NKF, kf_valid, kf_row, nn, nn2, Tcap):
    """gl_fuse_targets -> dict(tgt_kf (Tcap,), n_tgt (1,), result (4,)); entries beyond the list: 0"""
    tgt, bad = [], 0
    ok = lambda k: kf_valid is None or kf_valid[k]
    for k1 in g["cov_kf"][kf_row, :min(nn, _ord(g, kf_row))].tolist():
        if k1 < 0 or k1 >= NKF:
            bad += 1
            continue
        if not ok(k1) or k1 in tgt:
            continue
        tgt.append(k1)
        for k2 in g["cov_kf"][k1, :min(nn2, _ord(g, k1))].tolist():
            if k2 < 0 or k2 >= NKF:
                bad += 1
                continue
            if not ok(k2) or k2 in tgt or k2 == kf_row:
                continue
            tgt.append(k2)
    out = dict(tgt_kf=np.zeros(Tcap, np.int32), n_tgt=np.array([len(tgt)], np.int32))
    out["tgt_kf"][:min(len(tgt), Tcap)] = tgt[:Tcap]
    out["result"] = np.array([len(tgt), (LIST_TRUNCATED if len(tgt) > Tcap else 0) | (COVIS_BAD_ROW if bad else 0), 0, bad], np.int32)
    return out


def rows_candidates(m, tgt_kf, n_tgt, kf_idx, cand_cap):
    """gl_fuse_candidates, vectorised: the first position of every point over the (target, slot) grid -> dict(cand_mp (cand_cap,),
    n_cand (1,), result (4,)); entries beyond the list: 0"""
    NMP, (NKF, NFK) = len(m["mp_valid"]), m["kf_mp"].shape
    t = np.asarray(tgt_kf[:int(np.clip(n_tgt, 0, len(tgt_kf)))], np.int64)
    inside = (t >= 0) & (t < NKF)
    p = np.where(inside[:, None], m["kf_mp"][np.where(inside, t, 0)], -1).reshape(-1).astype(np.int64)
    good = (p >= 0) & (p < NMP)
    good &= m["mp_valid"][np.where(good, p, 0)] != 0
    pos = np.flatnonzero(good)
    first = np.full(NMP, np.iinfo(np.int64).max)
    np.minimum.at(first, p[pos], pos)
    cand = p[pos[first[p[pos]] == pos]] if kf_idx != 0 else p[:0]
    out = dict(cand_mp=np.zeros(cand_cap, np.int32), n_cand=np.array([len(cand)], np.int32))
    out["cand_mp"][:min(len(cand), cand_cap)] = cand[:cand_cap]
    nbad = int((~inside).sum())
    out["result"] = np.array([len(cand), (LIST_TRUNCATED if len(cand) > cand_cap else 0) | (COVIS_BAD_ROW if nbad else 0), 0, nbad], np.int32)
    return out
