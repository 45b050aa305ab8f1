"""The resident map's entry points - gl_update_connections, gl_ba_window_build, gl_cull_keyframes, gl_map_remove, gl_update_local_map,
gl_update_map_points - as hand-built cases: a few key-frames and points, the arguments, and every output array DECLARED by hand, one
case on either side of every decision (DECISIONS names the pairs).  tests/test_map_cases.py holds both forms of every restatement to
the declared outputs, tests/test_gpu_map_cases.py the device.  Test infrastructure: no GPU, nothing of the product is imported.

A case is Case(entry, m, ba, args, out): `m` / `ba` the map dicts of tests/ba_window_ref.py (for the point refresh: `kf` / `mp` of
tests/map_point_ref.py), `args` the call's other arguments, `out` the declaration in its shortest hand-written form; the *_arrays
functions below spell a declaration out as the buffers the device works on (sentinels behind every list's contents), nothing more.
The one table without a hand-written output is STRUCT (the two paths of rank_selected in gl_ba_window.hip): maps built by a function
around a hub key-frame, their outputs computed by connections_seq / window_seq, the line-by-line form of tests/ba_window_ref.py."""
import functools

import numpy as np

from tests import ba_window_ref as R

SENT = -7
KEPT, TRUNCATED = 1, 2                                        # gl_update_connections
NO_CONN, P_TRUNC, F_TRUNC, L_TRUNC, O_TRUNC = 1, 2, 4, 8, 16  # gl_ba_window_build; dropped << 8
JUDGED, FIRST = 0, 1                                          # gl_cull_keyframes
FIRST_REFUSED = 1                                             # gl_map_remove
LM_KEPT, LM_MP_TRUNCATED, LM_KF_TRUNCATED = 1, 2, 4           # gl_update_local_map
OBS = ("kf_mp", "obs_ptr", "obs_kf", "obs_feat")              # what an observation more or less changes in the inputs


class Case:
    def __init__(self, entry, m, ba, args, out):
        self.entry, self.m, self.ba, self.args, self.out = entry, m, ba, args, out

    def inputs(self):
        """every input array by name"""
        d = {k: v for k, v in self.m.items()}
        d.update(self.ba)
        d.update(self.args)
        return {k: np.asarray(v) for k, v in d.items() if v is not None}


def tiny_map(NKF, NFK, obs, stereo=True, oct_=None, first=0, invalid_mp=(), invalid_kf=(), extra_slots=None, assoc=None):
    """obs: per point a list of (key-frame, slot[, stereo]) in CSR order -> (m, ba).  extra_slots {(kf, slot): point}: a slot that holds
    a point whose entry list does not name the key-frame (what two gl_map_add triples onto one slot leave).  Every array the six entry
    points read is there: mp_pos = (p, 0.5, 2), kf_pose = (0 0 0 1, k 0 0), kf_uvr = (k, slot, 10 or -1), mp_assoc = 100 + p."""
    NMP = len(obs)
    kf_mp = -np.ones((NKF, NFK), np.int32)
    uvr = np.zeros((NKF, NFK, 3))
    uvr[:, :, 0], uvr[:, :, 1] = np.arange(NKF)[:, None], np.arange(NFK)[None]
    uvr[:, :, 2] = 10.0 if stereo else -1.0
    okf, of, ptr = [], [], [0]
    for p, lst in enumerate(obs):
        for e in lst:
            kf_mp[e[0], e[1]] = p
            okf.append(e[0])
            of.append(e[1])
            if len(e) > 2:
                uvr[e[0], e[1], 2] = 10.0 if e[2] else -1.0
        ptr.append(len(okf))
    for (k, f), p in (extra_slots or {}).items():
        kf_mp[k, f] = p
    mpv, kfv = np.ones(NMP, np.uint8), np.ones(NKF, np.uint8)
    mpv[list(invalid_mp)] = 0
    kfv[list(invalid_kf)] = 0
    pose = np.zeros((NKF, 7))
    pose[:, 3], pose[:, 4] = 1.0, np.arange(NKF)
    twc = np.zeros((NKF, 3))
    twc[:, 0] = -np.arange(NKF)
    a = np.arange(NMP, dtype=np.int32) + 100
    for p, v in (assoc or {}).items():
        a[p] = v
    m = dict(mp_valid=mpv, kf_valid=kfv, kf_mp=kf_mp, obs_ptr=np.array(ptr, np.int32), obs_kf=np.array(okf, np.int32),
             mp_pos=np.stack([np.arange(NMP, dtype=np.float64), np.full(NMP, 0.5), np.full(NMP, 2.0)], 1))
    ba = dict(kf_pose=pose, kf_twc=twc, kf_uvr=uvr, kf_oct=np.zeros((NKF, NFK), np.int32) if oct_ is None else np.array(oct_, np.int32),
              obs_feat=np.array(of, np.int32), mp_assoc=a, kf_first=first)
    return m, ba


# ================================================================================================ gl_update_connections
# key-frame 0 holds point p in slot p; observer k sees the first counts[k] of them, in slot p of its own

def conn_map(counts, NP=18, NKF=5, **kw):
    return tiny_map(NKF, NP, [[(0, p)] + [(k, p) for k in sorted(counts) if counts[k] > p] for p in range(NP)], **kw)


def CONN_(counts, lst, count, status=0, kf=0, Ccap=4, **kw):
    m, ba = conn_map(counts, **kw)
    return Case("conn", m, ba, dict(kf=kf, Ccap=Ccap), dict(list=lst, count=count, status=status))


CONN = {
    "count_14": CONN_({1: 14, 2: 16}, [(2, 16)], [0, 14, 16, 0, 0]),
    "count_15": CONN_({1: 15, 2: 16}, [(2, 16), (1, 15)], [0, 15, 16, 0, 0]),
    "none_at_15": CONN_({1: 14, 2: 9}, [(1, 14)], [0, 14, 9, 0, 0]),                  # the single largest is kept ...
    "one_at_15": CONN_({1: 15, 2: 9}, [(1, 15)], [0, 15, 9, 0, 0]),                   # ... and at 15 it is kept for its count
    "largest_tie": CONN_({1: 9, 2: 9}, [(1, 9)], [0, 9, 9, 0, 0]),                    # the lowest row of two largest below 15
    "largest_no_tie": CONN_({1: 8, 2: 9}, [(2, 9)], [0, 8, 9, 0, 0]),
    "equal_weights": CONN_({1: 15, 2: 17, 3: 15}, [(2, 17), (1, 15), (3, 15)], [0, 15, 17, 15, 0]),  # ascending rows below the larger weight
    "unequal_weights": CONN_({1: 15, 2: 17, 3: 16}, [(2, 17), (3, 16), (1, 15)], [0, 15, 17, 16, 0]),
    "own_not_counted": CONN_({1: 16}, [(1, 16)], [0, 16, 0, 0, 0]),                   # kf_count[0] = 0: it sees all 18 points itself
    "own_not_counted_from_1": CONN_({1: 16}, [(0, 16)], [16, 0, 0, 0, 0], kf=1),
    # point 0 also in slot 17 of key-frame 0 (nobody holds point 17 then): its two observers are counted twice
    "held_twice": CONN_({1: 14, 2: 16}, [(2, 17), (1, 15)], [0, 15, 17, 0, 0], extra_slots={(0, 17): 0}),
    "invalid_point": CONN_({1: 15, 2: 16}, [(2, 15)], [0, 14, 15, 0, 0], invalid_mp=[0]),
    "invalid_key_frame": CONN_({1: 15, 2: 16}, [(2, 16), (1, 15)], [0, 15, 16, 0, 0], invalid_kf=[1]),  # counted and listed
    "empty_counter": CONN_({}, [], [0, 0, 0, 0, 0], status=KEPT, NP=3),               # the lists stay as passed in
    "one_observation": CONN_({1: 1}, [(1, 1)], [0, 1, 0, 0, 0], NP=3),
    "ccap_below": CONN_({1: 15, 2: 17, 3: 15}, [(2, 17), (1, 15), (3, 15)], [0, 15, 17, 15, 0], status=TRUNCATED, Ccap=2),
    "ccap_equal": CONN_({1: 15, 2: 17, 3: 15}, [(2, 17), (1, 15), (3, 15)], [0, 15, 17, 15, 0], Ccap=3),
}


def conn_out(Ccap, NKF):
    return dict(conn_kf=np.full((1, Ccap), SENT, np.int32), conn_w=np.full((1, Ccap), SENT, np.int32), n_conn=np.full(1, SENT, np.int32),
                status=np.full(1, SENT, np.int32), kf_count=np.full((1, NKF), SENT, np.int32))


def conn_arrays(c):
    """the declaration as the device's buffers: the first Ccap rows of the list, its TRUE length, sentinels behind"""
    o, Ccap = c.out, c.args["Ccap"]
    a = conn_out(Ccap, len(o["count"]))
    n = min(len(o["list"]), Ccap)
    a["conn_kf"][0, :n], a["conn_w"][0, :n] = [k for k, _ in o["list"][:n]], [w for _, w in o["list"][:n]]
    a["n_conn"][0], a["status"][0], a["kf_count"][0] = len(o["list"]), o["status"], o["count"]
    return a


# ================================================================================================ gl_ba_window_build
# six key-frames of four slots, the window of key-frame 0.  Base: point 0 = kf 0, 1, 3; point 1 = kf 0, 1, 2; point 2 = kf 1, 3, 2:
# key-frame 1 shares two points with key-frame 0 (the single largest: free), 3 and 2 are first observed in that order (fixed).
W_BASE = [[(0, 0), (1, 0), (3, 0)], [(0, 1), (1, 1), (2, 0)], [(1, 2), (3, 1), (2, 1)]]
W_ROWS = [[(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (3, 0)], [(1, 2), (3, 1), (2, 1)]]     # the third observers swapped
W_SLOTS = [[(0, 1), (1, 0), (3, 0)], [(0, 0), (1, 1), (2, 0)], [(1, 2), (3, 1), (2, 1)]]    # key-frame 0 holds point 1 before point 0
W_KF2 = [[(0, 0), (2, 0), (3, 0)], [(0, 1), (2, 1), (1, 0)], [(2, 2), (3, 1), (1, 1)]]      # key-frames 1 and 2 change places
W_ALONE = [[(0, 0)], [(0, 1)]]
W_ALONE1 = [[(0, 0), (1, 0)], [(0, 1)]]
THREE = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]  # every CSR position of the base map, by point


def WIN_(obs, free, fixed, pts, edges, sizes, status=0, prior=None, caps=None, **kw):
    m, ba = tiny_map(6, 4, obs, **kw)
    caps = (4, 4, 6, 12) if caps is None else caps  # (room behind every list: the sentinels there must survive)
    prior = [1] + [0] * (len(free) - 1) if prior is None else prior
    return Case("window", m, ba, dict(kf=0, caps=caps), dict(free=free, fixed=fixed, pts=pts, obs=edges, prior=prior, sizes=sizes, status=status))


WINDOW = {
    "base": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9]),
    "fixed_in_row_order": WIN_(W_ROWS, [0, 1], [2, 3], [0, 1, 2], THREE, [2, 2, 3, 9]),
    # marked local but not free: its points (point 2) are not taken, it is not fixed, its observations make no edge
    "invalid_covisible": WIN_(W_BASE, [0], [3, 2], [0, 1], [[0, 2], [3, 5]], [1, 2, 2, 4], invalid_kf=[1]),
    "first_position": WIN_(W_SLOTS, [0, 1], [2, 3], [1, 0, 2], [[3, 4, 5], [0, 1, 2], [6, 7, 8]], [2, 2, 3, 9]),
    "other_free": WIN_(W_KF2, [0, 2], [3, 1], [0, 1, 2], THREE, [2, 2, 3, 9]),            # key-frame 1 observes and is not free: fixed
    "invalid_observer": WIN_(W_BASE, [0, 1], [2], [0, 1, 2], [[0, 1], [3, 4, 5], [6, 8]], [2, 1, 3, 7], invalid_kf=[3]),
    # point 3 sits in slot 2 of key-frame 0 and nobody observes it: no edge
    "no_edge_dropped": WIN_(W_BASE + [[]], [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], status=1 << 8, extra_slots={(0, 2): 3}, assoc={3: -1}),
    "no_edge_kept": WIN_(W_BASE + [[]], [0, 1], [3, 2], [0, 1, 3, 2], [[0, 1, 2], [3, 4, 5], [], [6, 7, 8]], [2, 2, 4, 9], extra_slots={(0, 2): 3}),
    "selected_invalid": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], [[1, 2], [4, 5], [6, 7, 8]], [2, 2, 3, 7], invalid_kf=[0]),  # free all the same
    "prior_on_second": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], prior=[0, 1], first=1),
    "prior_on_fixed": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], prior=[0, 0], first=3),  # kf_first is fixed: no flag
    "alone": WIN_(W_ALONE, [0], [], [0, 1], [[0], [1]], [1, 0, 2, 2], status=NO_CONN),
    "alone_plus_one": WIN_(W_ALONE1, [0, 1], [], [0, 1], [[0, 1], [2]], [2, 0, 2, 3]),
    "caps_equal": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], caps=(2, 2, 3, 9)),
    "pcap_below": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], status=P_TRUNC, caps=(1, 2, 3, 9)),
    "fcap_below": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], status=F_TRUNC, caps=(2, 1, 3, 9)),
    "lcap_below": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], status=L_TRUNC, caps=(2, 2, 2, 9)),
    "ocap_below": WIN_(W_BASE, [0, 1], [3, 2], [0, 1, 2], THREE, [2, 2, 3, 9], status=O_TRUNC, caps=(2, 2, 3, 8)),
}

SLAB_DTYPES = {"poses": np.float64, "prior": np.uint8, "points": np.float64, "assoc": np.int32, "obs_ptr": np.int32, "obs_pose": np.int32,
               "obs_uvr": np.float64, "obs_oct": np.int32, "win_kf": np.int32, "win_mp": np.int32, "win_obs": np.int32, "sizes": np.int32,
               "status": np.int32}


def empty_slab(caps):
    Pcap, Fcap, Lcap, Ocap = caps
    shapes = {"poses": (1, Pcap + Fcap, 7), "prior": (1, Pcap), "points": (1, Lcap, 3), "assoc": (1, Lcap), "obs_ptr": (1, Lcap + 1),
              "obs_pose": (1, Ocap), "obs_uvr": (1, Ocap, 3), "obs_oct": (1, Ocap), "win_kf": (1, Pcap + Fcap), "win_mp": (1, Lcap),
              "win_obs": (1, Ocap), "sizes": (1, 4), "status": (1,)}
    return {k: np.full(sh, 77 if k == "prior" else SENT, SLAB_DTYPES[k]) for k, sh in shapes.items()}


def window_arrays(c):
    """the declaration as a slab: the declared rows gathered from the map's arrays, cut at the capacities, sentinels behind; sizes and
    status as declared"""
    o, m, ba = c.out, c.m, c.ba
    Pcap, Fcap, Lcap, Ocap = c.args["caps"]
    s = empty_slab(c.args["caps"])
    order, flat = o["free"] + o["fixed"], [x for l in o["obs"] for x in l]
    n = min(len(order), Pcap + Fcap)
    s["win_kf"][0, :n], s["poses"][0, :n] = order[:n], ba["kf_pose"][order[:n]]
    n = min(len(o["free"]), Pcap)
    s["prior"][0, :n] = o["prior"][:n]
    L, n = len(o["pts"]), min(len(o["pts"]), Lcap)
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in o["obs"]])]).astype(np.int32)
    s["win_mp"][0, :n], s["points"][0, :n], s["assoc"][0, :n], s["obs_ptr"][0, :n] = o["pts"][:n], m["mp_pos"][o["pts"][:n]], ba["mp_assoc"][o["pts"][:n]], ptr[:n]
    if L <= Lcap:
        s["obs_ptr"][0, L] = len(flat)
    n = min(len(flat), Ocap)
    at = np.array(flat[:n], np.int64)
    k, f = m["obs_kf"][at], ba["obs_feat"][at]
    s["win_obs"][0, :n], s["obs_pose"][0, :n] = at, [order.index(int(x)) for x in k]
    s["obs_uvr"][0, :n], s["obs_oct"][0, :n] = ba["kf_uvr"][k, f].reshape(-1, 3), ba["kf_oct"][k, f]
    s["sizes"][0], s["status"][0] = o["sizes"], o["status"]
    return s


# ================================================================================================ gl_cull_keyframes
# all depths 1 and th_depth 6 but where a case says otherwise; octave 0; every observation stereo but where marked False

def CULL_(NKF, NFK, obs, cand, cull, mps, red, status=None, depth=None, **kw):
    m, ba = tiny_map(NKF, NFK, obs, **kw)
    d = np.ones((NKF, NFK), np.float32)
    for (k, f), v in (depth or {}).items():
        d[k, f] = v
    return Case("cull", m, ba, dict(cand=cand, kf_depth=d, th_depth=6.0),
                dict(cull=cull, num_mps=mps, num_redundant=red, status=[JUDGED] * len(cand) if status is None else status))


MONO3 = [(2, 0, False), (3, 0, False), (4, 0, False)]
EARLIER = [[(1, 0), (2, 0), (3, 0), (5, 1)], [(5, 0), (2, 1), (3, 1), (4, 1)]]
CASCADE = [[(1, 0), (2, 2), (3, 2)], [(5, 0), (2, 1), (3, 1), (4, 1)], [(1, 1), (5, 1)]]
CASCADE3 = CASCADE[:2] + [[(1, 1), (5, 1), (2, 0, False)]]


def ninety(n, redundant):
    """n counted points on key-frame 1, `redundant` of them with three other observers, the rest with two"""
    return [[(1, i), (2, i), (3, i)] + ([(4, i)] if i < redundant else []) for i in range(n)]


OCT_ = np.zeros((5, 2), np.int32)
OCT_[1] = 2
OCT_[2:, 0], OCT_[2:, 1] = 3, 4
FOUR = [[(1, i), (2, i), (3, i), (4, i)] for i in range(4)]

CULL = {
    # key-frame 1 holds point 0 in a slot, the point's entries name three others: w is theirs alone.  Three mono observers: w = 3, near = 3
    "w3": CULL_(6, 2, [MONO3], [1], [0], [1], [0], extra_slots={(1, 0): 0}),
    "w4": CULL_(6, 2, [[(2, 0, True)] + MONO3[1:]], [1], [1], [1], [1], extra_slots={(1, 0): 0}),  # one of them stereo: w = 4
    "self_adds_w": CULL_(6, 2, [[(1, 0, False)] + MONO3], [1], [1], [1], [1]),      # its own mono observation: w = 4, near still 3
    "near2": CULL_(6, 2, [[(1, 0), (2, 0), (3, 0)]], [1], [0], [1], [0]),          # w = 6, two others (the candidate is not one of them)
    "near3": CULL_(6, 2, [[(1, 0), (2, 0), (3, 0), (4, 0)]], [1], [1], [1], [1]),
    # key-frame 5 goes first and is culled: it no longer observes point 0 when key-frame 1 is judged (near 2) ...
    "culled_earlier": CULL_(6, 2, EARLIER, [5, 1], [1, 0], [2, 1], [2, 0]),
    "culled_later": CULL_(6, 2, EARLIER, [1, 5], [1, 0], [1, 2], [1, 1]),          # ... the other way round key-frame 1 still has it (near 3)
    # point 2 = kf 1, 5: the cull of key-frame 5 leaves it w = 2, dead, not in key-frame 1's num_mps; with a mono third observer: w = 3
    "cascade_w2": CULL_(6, 3, CASCADE, [5, 1], [1, 0], [1, 1], [1, 0], depth={(5, 1): -1.0}),
    "cascade_w3": CULL_(6, 3, CASCADE3, [5, 1], [1, 0], [1, 2], [1, 0], depth={(5, 1): -1.0}),
    "ninety_10_at": CULL_(5, 10, ninety(10, 9), [1], [0], [10], [9]),               # 9 > 0.9 * 10 is false
    "ninety_10_over": CULL_(5, 10, ninety(10, 10), [1], [1], [10], [10]),
    "ninety_1200_at": CULL_(5, 1200, ninety(1200, 1080), [1], [0], [1200], [1080]),  # the slot loop runs twice, the sum crosses all 16 waves
    "ninety_1200_over": CULL_(5, 1200, ninety(1200, 1081), [1], [1], [1200], [1081]),
    # depth exactly th_depth (slot 0) and depth 0 (slot 3) count, the next float above th_depth and -1 do not: two points, both redundant
    "depth_threshold": CULL_(5, 4, FOUR, [1], [1], [2], [2],
                             depth={(1, 0): 6.0, (1, 1): np.nextafter(np.float32(6.0), np.float32(7.0)), (1, 2): -1.0, (1, 3): 0.0}),
    # key-frame 1 sees both points at octave 2; point 0's other observers sit at octave 3 (counted), point 1's at 4 (not)
    "octave_plus_one": CULL_(5, 2, [[(1, 0), (2, 0), (3, 0), (4, 0)], [(1, 1), (2, 1), (3, 1), (4, 1)]], [1], [0], [2], [1], oct_=OCT_),
    "kf_first": CULL_(4, 4, [[(0, i), (1, i), (2, i), (3, i)] for i in range(4)], [0, 1], [0, 1], [0, 4], [0, 4], status=[FIRST, JUDGED]),
}


def cull_out(Ccap):
    out = {k: np.full((1, Ccap), 77 if k == "cull" else SENT, np.uint8 if k == "cull" else np.int32) for k in ("cull", "num_mps", "num_redundant", "cand_status", "cull_rows")}
    out["n_cull"] = np.full(1, SENT, np.int32)
    return out


def cull_arrays(c):
    """(cand (1, Ccap), n_cand (1,), the outputs): Ccap two above the list, sentinels behind; cull_rows = the culled candidates in order"""
    o, cand = c.out, c.args["cand"]
    n, Ccap = len(cand), len(cand) + 2
    a = cull_out(Ccap)
    a["cull"][0, :n], a["num_mps"][0, :n], a["num_redundant"][0, :n], a["cand_status"][0, :n] = o["cull"], o["num_mps"], o["num_redundant"], o["status"]
    rows = [k for k, v in zip(cand, o["cull"]) if v]
    a["cull_rows"][0, :len(rows)], a["n_cull"][0] = rows, len(rows)
    cd = np.full((1, Ccap), -3, np.int32)
    cd[0, :n] = cand
    return cd, np.array([n], np.int32), a


# ================================================================================================ gl_map_remove
def RM_(NKF, NFK, obs, ref, out, rm_mp=(), erase=(), rm_kf=(), **kw):
    m, ba = tiny_map(NKF, NFK, obs, **kw)
    i32 = lambda a: np.array(a, np.int32)
    args = dict(rm_mp=i32(rm_mp), erase=i32(erase), rm_kf=i32(rm_kf), mp_ref_kf=i32(ref))
    dt = dict(mp_valid=np.uint8, kf_valid=np.uint8)
    return Case("remove", m, ba, args, {k: (v if k == "status" else np.array(v, dt.get(k, np.int32)).reshape((NKF, NFK) if k == "kf_mp" else -1)) for k, v in out.items()})


THREE_OBS = [[(1, 0), (2, 0), (3, 0)]]
RANK_OBS = [[(1, 0), (2, 0), (3, 0, False), (4, 0, False)], [(3, 1), (4, 1), (0, 0)]]


def rank_out(kf3_slot0):
    return dict(mp_valid=[0, 1], kf_valid=[1, 0, 0, 0, 1], kf_mp=[[1, -1], [0, -1], [0, -1], [kf3_slot0, 1], [-1, 1]], obs_ptr=[0, 0, 2], obs_kf=[4, 0],
                obs_feat=[1, 0], obs_new_pos=[-1, -1, -1, -1, -1, 0, 1], dead_mp=[0], mp_ref_kf=[1, 4], status=0)


def three_out(kf_mp):
    return dict(mp_valid=[0], kf_valid=[1, 0, 0, 0], kf_mp=kf_mp, obs_ptr=[0, 0], obs_kf=[], obs_feat=[], obs_new_pos=[-1, -1, -1], dead_mp=[0], mp_ref_kf=[1], status=0)


REMOVE = {
    # point 0: two stereo observers (w = 4); point 1: two stereo + one mono (w = 5); the observation by key-frame 1 is erased from both:
    # the dead point keeps its mp_ref_kf entry, the survivor takes its first surviving observer
    "w4_dies_w5_survives": RM_(4, 2, [[(1, 0), (2, 0)], [(1, 1), (2, 1), (3, 0, False)]], [1, 1], erase=[0, 2], out=dict(
        mp_valid=[0, 1], kf_valid=[1, 1, 1, 1], kf_mp=[[-1, -1], [-1, -1], [-1, 1], [1, -1]], obs_ptr=[0, 0, 2], obs_kf=[2, 3], obs_feat=[1, 0],
        obs_new_pos=[-1, -1, -1, 0, 1], dead_mp=[0], mp_ref_kf=[1, 2], status=0)),
    # w = 6, all three removed: 6 -> 4 -> 2, the point dies at step 1; the first two removed keep their slot, the third is cleared
    "three_observers_123": RM_(4, 1, THREE_OBS, [1], rm_kf=[1, 2, 3], out=three_out([[-1], [0], [0], [-1]])),
    "three_observers_321": RM_(4, 1, THREE_OBS, [1], rm_kf=[3, 2, 1], out=three_out([[-1], [-1], [0], [0]])),
    # point 0: kf 1, 2 stereo, 3, 4 mono (w = 6); point 1: kf 3, 4, 0 stereo.  [1, 2, 3]: 6 -> 4 -> 2, point 0 dies at step 1 and key-frame
    # 3 (rank 2) is cleared; [3, 2, 1]: 6 -> 5 -> 3 -> 1, it dies at step 2 and no removed row is touched
    "rank_123": RM_(5, 2, RANK_OBS, [1, 3], rm_kf=[1, 2, 3], out=rank_out(-1)),
    "rank_321": RM_(5, 2, RANK_OBS, [1, 3], rm_kf=[3, 2, 1], out=rank_out(0)),
    "erased_to_w3": RM_(4, 1, [[(1, 0), (2, 0), (3, 0, False)]], [2], erase=[0], out=dict(
        mp_valid=[1], kf_valid=[1, 1, 1, 1], kf_mp=[[-1], [-1], [0], [0]], obs_ptr=[0, 2], obs_kf=[2, 3], obs_feat=[0, 0], obs_new_pos=[-1, 0, 1], dead_mp=[],
        mp_ref_kf=[2], status=0)),
    "erased_to_w2": RM_(4, 1, [[(1, 0), (2, 0)]], [2], erase=[0], out=dict(
        mp_valid=[0], kf_valid=[1, 1, 1, 1], kf_mp=[[-1], [-1], [-1], [-1]], obs_ptr=[0, 0], obs_kf=[], obs_feat=[], obs_new_pos=[-1, -1], dead_mp=[0],
        mp_ref_kf=[2], status=0)),
    "ref_lost": RM_(4, 1, THREE_OBS, [1], erase=[0], out=dict(
        mp_valid=[1], kf_valid=[1, 1, 1, 1], kf_mp=[[-1], [-1], [0], [0]], obs_ptr=[0, 2], obs_kf=[2, 3], obs_feat=[0, 0], obs_new_pos=[-1, 0, 1], dead_mp=[],
        mp_ref_kf=[2], status=0)),
    "ref_kept": RM_(4, 1, THREE_OBS, [1], erase=[1], out=dict(
        mp_valid=[1], kf_valid=[1, 1, 1, 1], kf_mp=[[-1], [0], [-1], [0]], obs_ptr=[0, 2], obs_kf=[1, 3], obs_feat=[0, 0], obs_new_pos=[0, -1, 1], dead_mp=[],
        mp_ref_kf=[1], status=0)),
    "kf_first_refused": RM_(4, 4, [[(0, i), (1, i), (2, i), (3, i)] for i in range(4)], [0, 0, 0, 0], rm_kf=[0], out=dict(
        mp_valid=[1] * 4, kf_valid=[1] * 4, kf_mp=[[0, 1, 2, 3]] * 4, obs_ptr=[0, 4, 8, 12, 16], obs_kf=[0, 1, 2, 3] * 4, obs_feat=[0] * 4 + [1] * 4 + [2] * 4 + [3] * 4,
        obs_new_pos=list(range(16)), dead_mp=[], mp_ref_kf=[0, 0, 0, 0], status=FIRST_REFUSED)),
}
ROW_KEYS = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat", "obs_new_pos", "dead_mp", "mp_ref_kf")


# ================================================================================================ gl_update_local_map
def rows_map(kf_rows, NMP, mp_valid=None, kf_valid=None):
    """kf_rows: per key-frame its mappoints_ (-1 = null); the observations follow from it"""
    kf_mp = np.array(kf_rows, np.int32)
    obs = [[k for k in range(len(kf_mp)) if p in kf_mp[k]] for p in range(NMP)]
    ptr = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    return dict(kf_mp=kf_mp, obs_ptr=ptr, obs_kf=np.array([k for o in obs for k in o], np.int32),
                mp_valid=None if mp_valid is None else np.array(mp_valid, np.uint8), kf_valid=None if kf_valid is None else np.array(kf_valid, np.uint8))


#            kf 0          kf 1          kf 2           kf 3
ROWS = [[0, 1, -1, 2], [1, 2, 3, -1], [4, -1, 1, -1], [5, 6, -1, -1]]
PREV = dict(prev_kf=(6, 7), prev_mp=(9,), prev_ref=5)  # what the lists hold on entry; -7 behind


def behind(lst, cap):
    return list(lst) + [SENT] * (cap - len(lst))


def LM_(feat_mp, out, rows=ROWS, NMP=7, KFcap=8, NPcap=16, **kw):
    out = dict(dict(status=0), **out)
    return Case("local", rows_map(rows, NMP, **kw), {}, dict(dict(feat_mp=feat_mp, KFcap=KFcap, NPcap=NPcap), **PREV), out)


LOCAL = {
    # point 0 (seen by kf 0 alone) held twice
    "held_twice": LM_([0, 0, -1], dict(feat_mp=[0, 0, -1], kf_count=[2, 0, 0, 0], ref_kf=0, n_local_kf=1, local_kf=behind([0, 7], 8), n_local_mp=3,
                                       local_mp=behind([0, 1, 2], 16))),
    # point 1 is invalid: both features lose it; point 4 is seen by kf 2, which holds 4 and the invalid 1
    "invalid_held_point": LM_([1, 4, -1, 1], dict(feat_mp=[-1, 4, -1, -1], kf_count=[0, 0, 1, 0], ref_kf=2, n_local_kf=1, local_kf=behind([2, 7], 8),
                                                  n_local_mp=1, local_mp=behind([4], 16)), mp_valid=[1, 0, 1, 1, 1, 1, 1]),
    # kf 1 sees all three (count 3) and is invalid: neither local nor the reference; point 3 is held by it alone
    "invalid_key_frame": LM_([1, 2, 3], dict(feat_mp=[1, 2, 3], kf_count=[2, 3, 1, 0], ref_kf=0, n_local_kf=2, local_kf=behind([0, 2], 8), n_local_mp=4,
                                             local_mp=behind([0, 1, 2, 4], 16)), kf_valid=[1, 0, 1, 1]),
    "all_counted_invalid": LM_([5, 6], dict(feat_mp=[5, 6], kf_count=[0, 0, 0, 2], ref_kf=5, n_local_kf=0, local_kf=behind([6, 7], 8), n_local_mp=0,
                                            local_mp=behind([9], 16)), kf_valid=[1, 1, 1, 0]),
    # points 7, 8: no observation (temporal points)
    "empty_counter": LM_([-1, 7, -1, 8], dict(feat_mp=[-1, 7, -1, 8], kf_count=[0] * 5, ref_kf=5, n_local_kf=2, local_kf=behind([6, 7], 8), n_local_mp=1,
                                              local_mp=behind([9], 16), status=LM_KEPT), rows=ROWS + [[-1, -1, -1, -1]], NMP=9),
    "holds_nothing": LM_([-1, -1], dict(feat_mp=[-1, -1], kf_count=[0] * 5, ref_kf=5, n_local_kf=2, local_kf=behind([6, 7], 8), n_local_mp=1,
                                        local_mp=behind([9], 16), status=LM_KEPT), rows=ROWS + [[-1, -1, -1, -1]], NMP=9),
    "tie_lowest_row": LM_([1], dict(feat_mp=[1], kf_count=[1, 1, 1, 0], ref_kf=0, n_local_kf=3, local_kf=behind([0, 1, 2], 8), n_local_mp=5,
                                    local_mp=behind([0, 1, 2, 3, 4], 16))),
    "tie_lowest_valid_row": LM_([1, 4, 3], dict(feat_mp=[1, 4, 3], kf_count=[1, 2, 2, 0], ref_kf=1, n_local_kf=2, local_kf=behind([1, 2], 8), n_local_mp=4,
                                                local_mp=behind([1, 2, 3, 4], 16)), kf_valid=[0, 1, 1, 1]),
    "shared_point_once": LM_([1], dict(feat_mp=[1], kf_count=[1, 1, 1, 0], ref_kf=0, n_local_kf=3, local_kf=behind([0, 1, 2], 8), n_local_mp=4,
                                       local_mp=behind([0, 1, 3, 4], 16)), mp_valid=[1, 1, 0, 1, 1, 1, 1]),
    "truncated_both": LM_([1], dict(feat_mp=[1], kf_count=[1, 1, 1, 0], ref_kf=0, n_local_kf=3, local_kf=[0, 1], n_local_mp=5, local_mp=[0, 1, 2],
                                    status=LM_MP_TRUNCATED | LM_KF_TRUNCATED), KFcap=2, NPcap=3),
    "truncated_points": LM_([1], dict(feat_mp=[1], kf_count=[1, 1, 1, 0], ref_kf=0, n_local_kf=3, local_kf=[0, 1, 2], n_local_mp=5, local_mp=[0, 1, 2, 3],
                                      status=LM_MP_TRUNCATED), KFcap=3, NPcap=4),
}
LOCAL_KEYS = ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "status", "kf_count")


def local_lists(c):
    """the lists on entry, as tests/test_local_map_ref.py always made them"""
    a = c.args
    KFcap, NPcap, pk, pm = a["KFcap"], a["NPcap"], a["prev_kf"], a["prev_mp"]
    lists = dict(local_kf=np.full((1, KFcap), SENT, np.int32), n_local_kf=np.array([len(pk)], np.int32), local_mp=np.full((1, NPcap), SENT, np.int32),
                 n_local_mp=np.array([len(pm)], np.int32), ref_kf=np.array([a["prev_ref"]], np.int32), status=np.array([SENT], np.int32),
                 kf_count=np.full((1, c.m["kf_mp"].shape[0]), SENT, np.int32))
    lists["local_kf"][0, :min(len(pk), KFcap)] = pk[:KFcap]
    lists["local_mp"][0, :min(len(pm), NPcap)] = pm[:NPcap]
    return lists


def local_arrays(c):
    o = c.out
    return np.array([o["feat_mp"]], np.int32), {k: np.array([o[k]], np.int32) for k in LOCAL_KEYS}


# ================================================================================================ gl_update_map_points
def prefix(b):
    """the first b bits set: two of them are |b1 - b2| apart"""
    bits = np.zeros(256, np.uint8)
    bits[:b] = 1
    return np.packbits(bits, bitorder="little")


def segment(lo, hi):
    """bits lo .. hi - 1 set: two disjoint ones are the sum of their lengths apart"""
    bits = np.zeros(256, np.uint8)
    bits[lo:hi] = 1
    return np.packbits(bits, bitorder="little")


PT_NKF, PT_NFK = 8, 4


def table(NKF=PT_NKF, NFK=PT_NFK):
    """key-frames 0 .. 7; kf k sits at (k + 1, 0, 0) except kf 1 at (0, -3, 0), kf 2 at (0, 0, -4) and kf 7 at the origin"""
    twc = np.array([[k + 1.0, 0.0, 0.0] for k in range(NKF)])
    twc[1], twc[2], twc[7] = [0.0, -3.0, 0.0], [0.0, 0.0, -4.0], [0.0, 0.0, 0.0]
    oct_ = np.tile(np.arange(NFK, dtype=np.int32), (NKF, 1))  # feature f has octave f
    return dict(twc=twc, valid=np.ones(NKF, np.uint8), oct=oct_, desc=np.zeros((NKF, NFK, 32), np.uint8))


def points(rows, ref=None, pos=None, valid=None):
    """rows: per point the list of (kf, feat)"""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = [o for r in rows for o in r]
    return dict(pos=np.zeros((len(rows), 3)) if pos is None else np.asarray(pos, np.float64),
                valid=np.ones(len(rows), np.uint8) if valid is None else np.asarray(valid, np.uint8),
                ref_kf=np.array([r[0][0] if r else 0 for r in rows] if ref is None else ref, np.int32), obs_ptr=ptr,
                obs_kf=np.array([k for k, _ in flat], np.int32), obs_feat=np.array([f for _, f in flat], np.int32))


def sentinel(NP):
    return dict(desc=np.full((NP, 32), 0xA5, np.uint8), normal=np.full((NP, 3), -7.0), max_dist=np.full(NP, -1.0, np.float32),
                min_dist=np.full(NP, -2.0, np.float32))


def with_descs(kf, kfs_bits):
    for k, f, b in kfs_bits:
        kf["desc"][k, f] = prefix(b)
    return kf


def scale_factors():
    """the float recurrence of the pyramid's scale factors at 1.2, 8 levels"""
    sf = [np.float32(1.0)]
    for _ in range(7):
        sf.append(np.float32(sf[-1] * np.float32(1.2)))
    return sf


SF = scale_factors()


def PT_(kf, mp, what, desc, normal=None, max_dist=None, min_dist=None, **edit):
    """desc: per point the prefix length of the declared descriptor, a (lo, hi) segment, or None: untouched; normal / max_dist / min_dist
    per point or None: untouched"""
    for k, v in edit.items():
        kf[k[:k.index("_at")]][v[0]] = v[1]
    return Case("points", kf, mp, dict(what=what), dict(desc=desc, normal=normal, max_dist=max_dist, min_dist=min_dist))


def _inv_table(v0):
    kf = with_descs(table(), [(0, 0, 7), (1, 0, 0), (2, 0, 10), (3, 0, 6)])
    kf["valid"][0] = v0
    return kf


INV_MP = dict(rows=[[(0, 0), (1, 0), (2, 0), (3, 0)]], ref=[1], pos=[[0.0, 0.0, 0.0]])
F3 = np.float32(3.0)

POINTS = {
    # N = 1: the descriptor; N = 2: medians 0 and 41, element (2 - 1) / 2 = 0 of each sorted row -> both 0, the first wins
    "n1_n2": PT_(with_descs(table(), [(0, 0, 5), (1, 1, 50), (2, 2, 9)]), points([[(0, 0)], [(1, 1), (2, 2)], [(2, 2), (1, 1)]]), 1, [5, 50, 9]),
    # N = 3, bits 0 / 10 / 6: rows {0,10,6} {10,0,4} {6,4,0}, element 1 of the sorted rows 6 / 4 / 4 -> row 1 (the first 4)
    # N = 4, bits 0 / 20 / 8 / 9: rows sorted {0,8,9,20} {0,11,12,20} {0,1,8,12} {0,1,9,11}, element 1: 8 / 11 / 1 / 1 -> row 2
    "n3_n4": PT_(with_descs(table(), [(0, 0, 0), (1, 0, 10), (2, 0, 6), (3, 0, 0), (4, 0, 20), (5, 0, 8), (6, 0, 9)]),
                 points([[(0, 0), (1, 0), (2, 0)], [(3, 0), (4, 0), (5, 0), (6, 0)]]), 1, [10, 8]),
    # bits 0 / 10 / 4: element 1 of the sorted rows {0,4,10} {0,6,10} {0,4,6} = 4 / 6 / 4: rows 0 and 2 tie, row 0 wins
    "median_tie": PT_(with_descs(table(), [(0, 0, 0), (1, 0, 10), (2, 0, 4)]), points([[(0, 0), (1, 0), (2, 0)]]), 1, [0]),
    # kf 0 invalid: the N = 3 case above on kf 1 .. 3; the normal counts it: kf 0 (1,0,0) -> (-1,0,0); kf 1 (0,-3,0) -> (0,1,0);
    # kf 2 (0,0,-4) -> (0,0,1); kf 3 (4,0,0) -> (-1,0,0); over n = 4.  |pos - Ow_ref| = 3, octave of feature 0 = 0
    "invalid_kf_skipped": PT_(_inv_table(0), points(**INV_MP), 3, [10], [[-0.5, 0.25, 0.25]], [F3], [np.float32(F3 / SF[7])]),
    # with kf 0: bits 7 / 0 / 10 / 6, element 1 of the sorted rows {0,1,3,7} {0,6,7,10} {0,3,4,10} {0,1,4,6} = 1 / 6 / 3 / 1 -> row 0
    "invalid_kf_valid": PT_(_inv_table(1), points(**INV_MP), 3, [7], [[-0.5, 0.25, 0.25]], [F3], [np.float32(F3 / SF[7])]),
    # the ref key-frame 5 at (6, 0, 0) does not observe the point: its feature 0 decides (octave 6)
    "ref_not_observed": PT_(table(), points([[(1, 3), (2, 1)]], ref=[5], pos=[[0.0, 0.0, 0.0]]), 2, [None], [[0.0, 0.5, 0.5]],
                            [np.float32(np.float32(6.0) * SF[6])], [np.float32(np.float32(np.float32(6.0) * SF[6]) / SF[7])], oct_at=(5, [6, 2, 2, 2])),
    # observed: the ref key-frame's own observation decides (feature 3 -> octave 3)
    "ref_observed": PT_(table(), points([[(1, 3), (2, 1)]], ref=[1], pos=[[0.0, 0.0, 0.0]]), 2, [None], [[0.0, 0.5, 0.5]],
                        [np.float32(F3 * SF[3])], [np.float32(np.float32(F3 * SF[3]) / SF[7])], oct_at=(5, [6, 2, 2, 2])),
    "at_camera_centre": PT_(table(), points([[(7, 0), (1, 0)]], ref=[1], pos=[[0.0, 0.0, 0.0]]), 2, [None], [[0.0, 0.5, 0.0]], [F3], [np.float32(F3 / SF[7])]),
    "only_at_camera_centre": PT_(table(), points([[(7, 0)]], ref=[7], pos=[[0.0, 0.0, 0.0]]), 2, [None], [[0.0, 0.0, 0.0]], [np.float32(0.0)], [np.float32(0.0)]),
    # 5 from kf 2 at (0, 0, -4), octave 7
    "octave_7": PT_(table(), points([[(2, 1)]], ref=[2], pos=[[0.0, 0.0, 1.0]]), 3, [0], [[0.0, 0.0, 1.0]], [np.float32(np.float32(5.0) * SF[7])],
                    [np.float32(np.float32(np.float32(5.0) * SF[7]) / SF[7])], oct_at=((2, 1), 7)),
    # octave 8, outside 0 .. 7: normal and depth untouched, the descriptor still written
    "octave_8": PT_(table(), points([[(2, 1)]], ref=[2], pos=[[0.0, 0.0, 1.0]]), 3, [0], oct_at=((2, 1), 8)),
}


def points_arrays(c):
    o = c.out
    NP = len(o["desc"])
    a = sentinel(NP)
    for p, d in enumerate(o["desc"]):
        if d is not None:
            a["desc"][p] = segment(*d) if isinstance(d, tuple) else prefix(d)
    for k in ("normal", "max_dist", "min_dist"):
        for p, v in enumerate(o[k] or []):
            if v is not None:
                a[k][p] = v
    return a


# ---- the descriptor sets: one map, a point per set.  Point c observes key-frames 0 .. N - 1, each at feature c, in list order.
# clusters(m): three groups of identical descriptors on disjoint segments of (m + 2) / 2, (m - 2) / 2 and m / 2 bits, so A-B = m, B-C = m - 1,
# A-C = m + 1.  With every group at most (N - 1) / 2 rows and any two together more, a row's element (N - 1) / 2 is its distance to the
# NEARER other group: A rows m, B rows m - 1, C rows m - 1.  A comes first and must not win; the first B row does.  3 m / 2 <= 256 bits
# hold m up to 170 - and no three descriptors of 256 bits are mutually more than 170 apart, so no tighter case exists above that.
def clusters(m, nA, nB, nC):
    a, b = (m + 2) // 2, (m - 2) // 2
    A, B, C = (0, a), (a, a + b), (a + b, a + b + m // 2)
    return [A] * nA + [B] * nB + [C] * nC, B, sorted({m, m - 1})


# sides(x): 16 rows at prefix(0) in front, 16 at prefix(256), one at prefix(x) last, x >= 128: the front rows' element 16 is x (their
# distance to the last row), the rows at 256 have 256 - x and win, the last row ties with them.  x = 256: 17 rows at 256, median 0
def sides(x):
    return [(0, 0)] * 16 + [(0, 256)] * 16 + [(0, x)], (0, 256), sorted({x, 256 - x})


def _desc_sets():
    sets = {"n3_far_apart": ([(0, 86), (86, 171), (171, 256)], (86, 171), [170, 171]),  # A-B = A-C = 171, B-C = 170: medians 171 / 170 / 170
            "distance_256": ([(0, 0), (0, 256), (0, 256)], (0, 256), [0, 256]),         # row 0: {0, 256, 256} -> 256; rows 1, 2: {0, 0, 256} -> 0
            "tie_first_of_three": ([(0, 0), (0, 10), (0, 4)], (0, 0), [4, 6])}           # the moved median_tie, in the shared map
    for N, (nA, nB, nC), m in ((32, (10, 11, 11), 96), (33, (11, 11, 11), 96), (64, (21, 21, 22), 112), (65, (21, 22, 22), 112), (128, (42, 43, 43), 144),
                               (129, (43, 43, 43), 160)):
        sets["n%d" % N] = clusters(m, nA, nB, nC)
    for m in range(16, 161, 16):
        sets["edge_%d" % m] = clusters(m, 11, 11, 11)
    for m in range(176, 257, 16):
        sets["edge_%d_below" % m], sets["edge_%d" % m] = sides(m - 1), sides(m)
    return sets


DESC_SETS = _desc_sets()  # name -> (the rows' segments in list order, the declared winner's segment, the row medians that occur)
DESC_NKF = 129


@functools.lru_cache(maxsize=None)
def desc_map():
    """-> (kf, mp, names): every set a point of one map"""
    names = list(DESC_SETS)
    kf = dict(twc=np.zeros((DESC_NKF, 3)), valid=np.ones(DESC_NKF, np.uint8), oct=np.zeros((DESC_NKF, len(names)), np.int32),
              desc=np.zeros((DESC_NKF, len(names), 32), np.uint8))
    rows = []
    for c, name in enumerate(names):
        segs = DESC_SETS[name][0]
        for k, s in enumerate(segs):
            kf["desc"][k, c] = segment(*s)
        rows.append([(k, c) for k in range(len(segs))])
    return kf, points(rows), names


def desc_case(name=None):
    """the set `name` alone (a map of one point), or all of them in one call"""
    kf, mp, names = desc_map()
    if name is None:
        return Case("points", kf, mp, dict(what=1), dict(desc=[DESC_SETS[n][1] for n in names], normal=None, max_dist=None, min_dist=None))
    c = names.index(name)
    n = len(DESC_SETS[name][0])
    one = points([[(k, c) for k in range(n)]])
    return Case("points", kf, one, dict(what=1), dict(desc=[DESC_SETS[name][1]], normal=None, max_dist=None, min_dist=None))


# ================================================================================================ rank_selected: the structural cases
# name -> (K, NKF, points of the hub, shuffled).  A hub key-frame 0 whose points are all seen by key-frames 1 .. K.  15 points: every
# weight is 15, the covisible list is rows 1 .. K ascending (K selected: at most 1 024 are ranked in LDS, more over the whole table).
# 14 points: nobody reaches 15, the single largest (row 1 of the tie) is the one free neighbour, P = 2, and the other K - 1 observers
# are fixed in the order of their first observation - the first point's entries are shuffled, so that is not the row order.  NKF up
# to 4 096: the per-key-frame words are in LDS, 4 097: in global memory.
STRUCT = {
    "list_1023": (1023, 1100, 15, False), "list_1024": (1024, 1100, 15, False), "list_1025": (1025, 1100, 15, False), "list_1025_global": (1025, 4097, 15, False),
    "fixed_1023": (1024, 1100, 14, True), "fixed_1024": (1025, 1100, 14, True), "fixed_1025": (1026, 1100, 14, True), "fixed_1025_global": (1026, 4097, 14, True),
}
STRUCT_NFK = 16


@functools.lru_cache(maxsize=None)
def struct_case(name):
    """-> dict(m, ba, kf = 0, K, conn = connections_seq's lists, win = window_seq's window, computed here, not written by hand)"""
    K, NKF, npts, shuffled = STRUCT[name]
    rng = np.random.default_rng(K + NKF)
    obs = []
    for p in range(npts):
        order = rng.permutation(K) + 1 if shuffled and p == 0 else np.arange(1, K + 1)
        obs.append([(0, p)] + [(int(k), p) for k in order])
    m, ba = tiny_map(NKF, STRUCT_NFK, obs)
    return dict(m=m, ba=ba, kf=0, K=K, conn=R.connections_seq(m, 0), win=R.window_seq(m, ba, 0))


# ================================================================================================ the decisions
# (entry, the decision, the case below it, the case above it, the declared outputs that differ, the inputs that differ).  An empty
# tuple of outputs: the two declarations are EQUAL, which is what the rule says (validity of a key-frame does not matter to the counter).
DECISIONS = [
    ("conn", "a count of 14 against 15", "count_14", "count_15", ("list", "count"), OBS),
    ("conn", "no observer at 15: the single largest is kept", "none_at_15", "one_at_15", ("list", "count"), OBS),
    ("conn", "two observers share the largest count below 15: the lowest row", "largest_no_tie", "largest_tie", ("list", "count"), OBS),
    ("conn", "equal weights at or above 15 in ascending row order, below any larger weight", "equal_weights", "unequal_weights", ("list", "count"), OBS),
    ("conn", "the key-frame's own observations are not counted", "own_not_counted", "own_not_counted_from_1", ("list", "count"), ("kf",)),
    ("conn", "a point held in two slots counts twice", "count_14", "held_twice", ("list", "count"), ("kf_mp",)),
    ("conn", "an invalid point is not counted", "invalid_point", "count_15", ("list", "count"), ("mp_valid",)),
    ("conn", "an invalid key-frame is counted and listed", "invalid_key_frame", "count_15", (), ("kf_valid",)),
    ("conn", "an empty counter gives GL_CONN_KEPT and leaves the lists", "empty_counter", "one_observation", ("list", "count", "status"), OBS),
    ("conn", "Ccap one below the list length, and equal to it", "ccap_below", "ccap_equal", ("status",), ("Ccap",)),
    ("window", "an invalid key-frame in the covisible list is marked, not free, its points not taken, never fixed", "invalid_covisible", "base",
     ("free", "pts", "obs", "sizes", "prior"), ("kf_valid",)),
    ("window", "a point held by two free key-frames is listed once, at its first position", "base", "first_position", ("pts", "obs", "fixed"), ("kf_mp", "obs_feat")),
    ("window", "fixed key-frames in order of their first observation, not in row order", "base", "fixed_in_row_order", ("fixed",), ("kf_mp", "obs_kf")),
    ("window", "an observer that is already free is not fixed", "base", "other_free", ("free", "fixed"), ("kf_mp", "obs_kf")),
    ("window", "an invalid observer makes no edge", "invalid_observer", "base", ("fixed", "obs", "sizes"), ("kf_valid",)),
    ("window", "a point with no edge is dropped when mp_assoc < 0 and kept otherwise", "no_edge_dropped", "no_edge_kept", ("pts", "obs", "sizes", "status"), ("mp_assoc",)),
    ("window", "the selected key-frame is itself invalid", "selected_invalid", "base", ("obs", "sizes"), ("kf_valid",)),
    ("window", "the prior flag sits on kf_first", "base", "prior_on_second", ("prior",), ("kf_first",)),
    ("window", "the prior flag only among the free poses", "prior_on_second", "prior_on_fixed", ("prior",), ("kf_first",)),
    ("window", "NO_CONN with a window of the key-frame alone", "alone", "alone_plus_one", ("free", "obs", "sizes", "status", "prior"), OBS),
    ("window", "P one above its capacity and equal to it", "pcap_below", "caps_equal", ("status",), ("caps",)),
    ("window", "F one above its capacity and equal to it", "fcap_below", "caps_equal", ("status",), ("caps",)),
    ("window", "L one above its capacity and equal to it", "lcap_below", "caps_equal", ("status",), ("caps",)),
    ("window", "nobs one above its capacity and equal to it", "ocap_below", "caps_equal", ("status",), ("caps",)),
    ("cull", "a point's weight w = 3 against w = 4", "w3", "w4", ("cull", "num_redundant"), ("kf_uvr",)),
    ("cull", "2 against 3 near observers", "near2", "near3", ("cull", "num_redundant"), OBS),
    ("cull", "the candidate itself adds to w", "w3", "self_adds_w", ("cull", "num_redundant"), ("obs_ptr", "obs_kf", "obs_feat", "kf_uvr")),
    ("cull", "the candidate itself does not add to near", "near2", "near3", ("cull", "num_redundant"), OBS),
    ("cull", "an observer culled earlier in the same list adds to neither", "culled_earlier", "culled_later", ("num_mps", "num_redundant"), ("cand",)),
    ("cull", "a point left with w <= 2 by an earlier cull is not in num_mps", "cascade_w2", "cascade_w3", ("num_mps",), OBS + ("kf_uvr",)),
    ("cull", "the 90 % boundary at num_mps = 10", "ninety_10_at", "ninety_10_over", ("cull", "num_redundant"), OBS),
    ("cull", "the 90 % boundary at num_mps = 1 200", "ninety_1200_at", "ninety_1200_over", ("cull", "num_redundant"), OBS),
    ("remove", "a stereo point erased down to w = 3 survives, down to w = 2 dies", "erased_to_w2", "erased_to_w3",
     ("mp_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat", "obs_new_pos", "dead_mp"), OBS + ("kf_uvr",)),
    ("remove", "mp_ref_kf moves only when the reference observer is lost", "ref_kept", "ref_lost", ("mp_ref_kf", "kf_mp", "obs_kf", "obs_new_pos"), ("erase",)),
    ("remove", "three observers in both orders", "three_observers_123", "three_observers_321", ("kf_mp",), ("rm_kf",)),
    ("remove", "the rank decides the removed rows", "rank_123", "rank_321", ("kf_mp",), ("rm_kf",)),
]
TABLES = dict(conn=CONN, window=WINDOW, cull=CULL, remove=REMOVE, local=LOCAL, points=POINTS)
