"""A mapping session - Localization::spinOnce (localization.cpp:65-110) for consecutive key-frames on ONE resident map - stated once: the
executable statement of the call order a host follows.  Test infrastructure; nothing in the product imports it.

Per arriving key-frame K (its kf_mp row filled by the tracking thread - followed one step through mp_replaced, as gl_track_frame_next
hands rows over -, nothing observes it, invalid; its table rows are the one upload) the steps of STEPS run in order, each a named function
of the model leg (m_*: every integer edit by the sequential models of tests/map_stats_ref.py - which inherits map_grow_ref and
map_edit_ref -, tests/covis_ref.py and frame_step_ref.note_replaced, on the host) and of the device leg (d_*: the product's entry points
and composites on one set of capacity buffers):

  0   a tracked frame's counters                       map_stats_track                          tracking.cpp:213-292
  1   processNewKeyFrame (localization.cpp:412-444): 1a the BoW row (bow.transform_into_tables), 1b map_add(new_kf = walk_kf = [K]),
      1c already_mp -> candidate_mappts_ (map_cand_append), 1d the refresh of the points that gained the observation, 1e gl_covis_update(K)
  2   removeMapPoints (:127-152)                       map_stats.remove_map_points_from_map
  3   createMapPoints (localization_opt.cpp:206-454)   map_grow.create_map_points_from_map, then map_stats_new_points + map_cand_append
  4   searchInNeighbors (:154-224)                     covis.search_in_neighbors_from_map with stats, mp_replaced and mp_ref_kf
  5   jointOptimization (localization_opt.cpp:456-925) 5a api.joint_optimization_from_map, 5c map_remove(erase_obs) (:884-894),
                                                       5b updateNormalAndDepth of the window's points (:914-922)
  6   removeKeyFrames (:334-399) + Map::removeKeyFrame 6a update_connections, 6b cull_keyframes, 6c map_remove(rm_kf), 6d covis_remove

ORDER.  5c runs before 5b: the reference erases the outlier observations (:884-894) before it recovers the points and calls
updateNormalAndDepth (:914-922), so the normals are those of the observations that are left.
DECLARED DEVIATIONS of the composites, counted by the model leg (events stale_nn_list / stale_cull_list) and reported by the tests:
createMapPoints reads curr_kf_->getBestCovisibilityKeyFrames(10) - the list updateConnections stored in step 1e, BEFORE removeMapPoints
(localization_opt.cpp:219) - and removeKeyFrames reads getVectorCovisibleKeyFrames() - the list stored at the end of step 4, BEFORE the
BA's erasures (localization.cpp:341); create_map_points_from_map and the route of api.mapping_pass_from_map count the connections
afresh on the map as it is (api.update_connections).  The two differ only where a removal in between moves a weight across 15 or past
a neighbour's.

The float producers (best_idx of the fuse search, createMapPoints' lists, the BA's poses / points / dropped / erase flags,
update_map_points) come from a `producers` object: OracleProducers (the C++ oracle and the numpy restatements the per-call *_ref tests use;
CPU) or DeviceProducers (the device on a map uploaded afresh before each of them, as host_pass of tests/test_gpu_map_grow.py does).  No
step of the model leg reads the device leg's state."""
import collections

import numpy as np

from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import bow_ref as BR
from tests import covis_ref as CR
from tests import create_points_ref as CP
from tests import frame_step_ref as FR
from tests import map_edit_ref as E
from tests import map_grow_ref as G
from tests import map_point_ref as MP
from tests import map_stats_ref as MS
from tests import session_scenes as SS

STEPS = ("0 track", "1a bow", "1b add", "1c candidates", "1d refresh", "1e covis", "2 remove points", "3 create points", "4 search in neighbours",
         "5a ba", "5c erase", "5b refresh", "6 remove key-frames")
NN, CCAP, COV_CCAP = 10, 64, 256       # createMapPoints' neighbours, the cull's list capacity, gl_covis_update's
CSR_KEYS = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")
FV_KEYS = ("nnode", "node_id", "node_ptr", "node_idx")
GRAPH_KEYS = ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov")
POINT_SPEC = (("mp_desc", np.uint8, (32,)), ("mp_normal", np.float64, (3,)), ("mp_max_dist", np.float32, ()), ("mp_min_dist", np.float32, ()))
BA_CAPS = (32, 32, 2048, 16384)
f32 = np.float32


def default_mb(cam):
    return float(f32(cam.bf) / f32(cam.fx))


# ---------------------------------------------------------------------------------------------------------------- the host's state
class Host:
    """the map, its counters, graph and tables as numpy arrays cut to the sizes; `events` counts what the session exercised"""

    def __init__(self, sc, P):
        self.sc, self.P = sc, P
        m, ba = sc["m"], sc["ba"]
        NMP = len(m["mp_valid"])
        self.m = {k: np.array(m[k]) for k in CSR_KEYS + ("mp_pos",)}
        for k, dt, sh in POINT_SPEC:
            self.m[k] = np.zeros((NMP,) + sh, dt)
        self.ba = {k: np.array(ba[k]) for k in SS.BA_ROW_KEYS + ("obs_feat", "mp_assoc")}
        self.ba["kf_first"] = int(ba["kf_first"])
        self.ref = np.array(sc["ref"], np.int32)
        st = sc["stats"]
        self.visible, self.found, self.ref_idx = (np.array(st[k], np.int32) for k in ("visible", "found", "ref_idx"))
        self.cand = [int(v) for v in st["cand"]]
        self.rep = -np.ones(NMP, np.int32)
        NKF, NFK = sc["NKF"], sc["NFK"]
        self.tree = BR.Tree(sc["voc"])
        self.kt = {k: np.zeros((NKF,) + v.shape[1:], v.dtype) for k, v in sc["kt"].items()}
        for k, v in sc["kt"].items():
            self.kt[k][:len(v)] = v
        self.kt.update(nnode=np.zeros(NKF, np.int32), node_id=np.zeros((NKF, NFK), np.int32), node_ptr=np.zeros((NKF, NFK + 1), np.int32),
                       node_idx=np.zeros((NKF, NFK), np.int32))
        self.kf_depth = np.full((NKF, NFK), -1.0, f32)
        self.kf_depth[:len(sc["kf_depth"])] = sc["kf_depth"]
        self.events = collections.Counter()
        self.need = collections.Counter()  # the largest need of every capacity
        self.nobs_trace, self.kept_before = [], set()
        for k in range(len(self.m["kf_valid"])):
            self._bow_row(k)
        self.G, self.g = CR.Model(NKF), None
        self.g = self.G.rows(NKF, fill=0)
        self.g["best_cov"][:] = -1
        for k in np.nonzero(self.m["kf_valid"])[0]:
            self.G.update_connections(self.m, int(k))
            CR.rows_update(self.g, self.m, int(k), COV_CCAP)
        self.graph_agrees("entry")
        P.refresh(self, self.m["mp_valid"] != 0, 3)
        self.note_need()

    # ---- sizes, views
    @property
    def sizes(self):
        return len(self.m["mp_valid"]), len(self.m["kf_valid"]), len(self.m["obs_kf"])

    def kt_view(self):
        NKF = self.sizes[1]
        return {k: v[:NKF] for k, v in self.kt.items()}

    def model(self):
        return MS.Model(self.m, self.ba, self.ref).set_stats(self.visible, self.found, self.ref_idx, None, self.cand)

    def take(self, M, rows):
        """the model's rows and counters become the state; its own consistency check runs on what every step leaves"""
        M.check_consistent()
        self.m.update({k: np.asarray(rows[k]) for k in CSR_KEYS})
        self.ba["obs_feat"] = np.asarray(rows["obs_feat"])
        self.ref = np.asarray(rows["mp_ref_kf"], np.int32)
        self.visible, self.found, self.ref_idx = M.stats_arrays()
        self.cand = list(M.cand)
        self.events.update(M.events)
        self.note_need()

    def note_need(self):
        NMP, NKF, NOBS = self.sizes
        for k, v in (("NMP", NMP), ("NOBS", NOBS), ("cand", len(self.cand)), ("W", int(self.g["cov_n"].max()))):
            self.need[k] = max(self.need[k], v)
        self.nobs_trace.append(NOBS)

    def _bow_row(self, k):
        r = BR.transform_batch(self.tree, self.kt["desc"][k:k + 1], None, 4, self.kt["node_id"].shape[1], 0)
        assert int(r["status"][0]) == 0
        for key in FV_KEYS:
            self.kt[key][k] = r[key][0]

    def graph_agrees(self, what):
        """the object model and the row representation say the same graph"""
        ref = self.G.rows(self.g["cov_kf"].shape[1])
        for k in range(len(self.G.kfs)):
            n = int(ref["cov_n"][k])
            assert n == self.g["cov_n"][k] and ref["cov_nord"][k] == self.g["cov_nord"][k] and ref["best_cov"][k] == self.g["best_cov"][k], (what, k)
            assert np.array_equal(ref["cov_kf"][k, :n], self.g["cov_kf"][k, :n]) and np.array_equal(ref["cov_w"][k, :n], self.g["cov_w"][k, :n]), (what, k)

    def covis_update(self, K):
        self.G.update_connections(self.m, K)
        out = CR.rows_update(self.g, self.m, K, COV_CCAP)
        assert not out["result"][1] & CR.W_TRUNCATED
        self.need["W"] = max(self.need["W"], int(out["result"][0]))
        self.graph_agrees(("update", K))
        return out

    def snapshot(self):
        NMP, NKF, NOBS = self.sizes
        s = {k: self.m[k].copy() for k in self.m}
        s.update({k: self.ba[k].copy() for k in self.ba if k != "kf_first"})
        s.update(mp_ref_kf=self.ref.copy(), visible=self.visible.copy(), found=self.found.copy(), ref_idx=self.ref_idx.copy(),
                 cand=np.array(self.cand, np.int32), mp_replaced=self.rep.copy(), sizes=np.array(self.sizes, np.int32))
        s.update({k: v.copy() for k, v in self.g.items()})
        s.update({"kt_" + k: self.kt[k].copy() for k in FV_KEYS})
        return s


# ---------------------------------------------------------------------------------------------------------------- the model leg's steps
def arrive(H, K):
    """key-frame K handed over: its rows appended, the kf_mp row followed one step through mp_replaced, invalid, nothing observes it"""
    row = H.sc["rows"][K]
    NMP = H.sizes[0]
    held = row["kf_mp"].astype(np.int64)
    ok = (held >= 0) & (held < NMP)
    to = np.where(ok, H.rep[np.where(ok, held, 0)], -1)
    H.events["arrival_followed_replaced"] += int((to >= 0).sum())
    kf_mp = np.where(to >= 0, to, held).astype(np.int32)
    assert H.sizes[1] == K
    H.m["kf_mp"] = np.concatenate([H.m["kf_mp"], kf_mp[None]])
    H.m["kf_valid"] = np.concatenate([H.m["kf_valid"], np.zeros(1, np.uint8)])
    for key in SS.BA_ROW_KEYS:
        H.ba[key] = np.concatenate([H.ba[key], row[key][None]])
    for key in SS.KT_ROW_KEYS:
        H.kt[key][K] = row[key]
    H.kf_depth[K] = row["kf_depth"]
    return dict(kf_mp=kf_mp)


def m_track(H, K):
    a = SS.track_inputs(H.sc, K, H.m, H.m["kf_mp"][K])
    M = H.model()
    MS.model_track(M, **a)
    vis, fnd = MS.track(H.visible, H.found, H.sizes[0], **a)  # (the call stated directly: the inputs are what the chain would leave)
    H.visible, H.found, H.ref_idx = M.stats_arrays()
    assert np.array_equal(vis, H.visible) and np.array_equal(fnd, H.found)
    H.events.update(M.events)
    return dict(inputs=a)


def m_bow(H, K):
    H._bow_row(K)
    return {}


def m_add(H, K):
    M = H.model()
    rows, res = G.map_add(H.m, H.ba, H.ref, None, [K], (), [K], model=M)
    assert res[5] == 0
    H.take(M, rows)
    H.already = rows["already_mp"]
    H.events["walk_attached"] += res[2]
    H.events["walk_already"] += res[4]
    return dict(n_attached=res[2], n_skipped=res[3], n_already=res[4], status=res[5], already_mp=rows["already_mp"])


def m_candidates(H, K):
    H.cand += [int(v) for v in H.already]
    H.note_need()
    return {}


def held_valid(H, rows):
    NMP = H.sizes[0]
    mask = np.zeros(NMP, bool)
    rows = np.asarray(rows, np.int64)
    mask[rows[(rows >= 0) & (rows < NMP)]] = True
    return mask & (H.m["mp_valid"] != 0)


def m_refresh_row(H, K):
    H.P.refresh(H, held_valid(H, H.m["kf_mp"][K]), 3)
    return {}


def m_covis(H, K):
    return dict(H.covis_update(K))


def m_remove_points(H, K):
    M = H.model()
    old = list(H.cand)
    met = [p for p in old if p in H.kept_before]
    verdict, removed = M.remove_map_points(K)
    rows = M.to_rows()
    H.take(M, rows)
    H.events["mp_removed"] += len(removed)
    H.events["kept_met_again"] += len(met)
    H.kept_before |= set(H.cand)
    return dict(verdict=np.array(verdict, np.int32), rm_mp=np.array(removed, np.int32), dead_mp=np.array(sorted(M.dead), np.int32),
                result=np.array([len(H.cand), len(removed), len(old) - len(H.cand) - len(removed), 0], np.int32), nobs=H.sizes[2])


def m_create_points(H, K):
    NMP = H.sizes[0]
    c = R.connections_vec(H.m, K)
    conn = -np.ones(NN, np.int32)
    conn[:min(NN, len(c["conn_kf"]))] = c["conn_kf"][:NN]
    stored = H.G.best_covisibles(K, NN)[0]
    H.events["stale_nn_list"] += list(stored) != c["conn_kf"][:NN].tolist()
    s = H.P.create(H, K, conn, len(c["conn_kf"]))
    n = int(s["n_new"])
    M = H.model()
    new = dict(pos=s["new_pos"][:n], assoc=s["new_assoc"][:n], ref_kf=s["new_ref_kf"][:n])
    att = np.stack([s["att_mp"][:2 * n], s["att_kf"][:2 * n], s["att_feat"][:2 * n]], 1).reshape(-1, 3)
    rows, res = G.map_add(H.m, H.ba, H.ref, new, (), att, (), model=M)
    assert res[5] == 0 and res[0] == NMP + n
    H.m["mp_pos"] = np.concatenate([H.m["mp_pos"], np.asarray(new["pos"], np.float64).reshape(n, 3)])
    for k, dt, sh in POINT_SPEC:
        H.m[k] = np.concatenate([H.m[k], np.zeros((n,) + sh, dt)])
    H.ba["mp_assoc"] = np.concatenate([H.ba["mp_assoc"], np.asarray(new["assoc"], np.int32)])
    H.rep = np.concatenate([H.rep, -np.ones(n, np.int32)])
    H.take(M, rows)
    H.cand += list(range(NMP, NMP + n))
    H.note_need()
    mask = np.zeros(NMP + n, bool)
    mask[NMP:] = True
    H.P.refresh(H, mask & (H.m["mp_valid"] != 0), 3)
    made = s["nb_stats"][:, 3]
    H.events["created"] += n
    H.events["created_at_two_neighbours"] += int((made > 0).sum() >= 2)
    searched = np.nonzero(s["nb_stats"][:, 1] == 0)[0]
    H.events["created_feature_is_no_query_later"] += int(sum(made[j] for j in searched[:-1]))
    return dict(n_new=n, new_type=s["new_type"][:n], new_nb=s["new_nb"][:n], feat_new=s["feat_new"], nb_stats=s["nb_stats"], n_attached=res[2],
                n_skipped=res[3], status=res[5])


def m_fuse(H, kf, cand, counts):
    cand = np.asarray(cand, np.int32)
    H.need["NOBS"] = max(H.need["NOBS"], H.sizes[2] + len(cand))  # (gl_map_fuse wants room for every candidate to attach)
    best = H.P.fuse_best(H, kf, cand)
    M = H.model()
    rows, res = G.map_fuse(H.m, H.ba, kf, cand, best, model=M)
    H.take(M, rows)
    for k, v in zip(("n_fused", "n_attached", "n_replaced"), res[1:4]):
        counts[k].append(int(v))
    H.events["fuse_attached"] += res[2]
    H.events["fuse_replaced"] += res[3]
    src, tgt = rows["repl_src"], rows["repl_tgt"]
    if len(src):
        H.P.refresh(H, held_valid(H, tgt), 1)
        H.rep = FR.note_replaced(H.rep, src, tgt)


def m_search_in_neighbours(H, K):
    targets = H.G.fuse_targets(K, H.m["kf_valid"], NN, 5)
    t2 = CR.rows_targets(H.g, H.sizes[1], H.m["kf_valid"], K, NN, 5, NN + NN * 5)
    assert t2["tgt_kf"][:int(t2["n_tgt"][0])].tolist() == targets
    H.events["targets_after_a_cull"] += int(H.events["kf_culled"] > 0 and len(targets) > 0)
    snapshot = H.m["kf_mp"][K].copy()
    counts = dict(n_fused=[], n_attached=[], n_replaced=[])
    for t in targets:
        m_fuse(H, t, snapshot, counts)
    cand = CR.fuse_candidates(H.m, targets, K)
    m_fuse(H, K, cand, counts)
    H.P.refresh(H, held_valid(H, H.m["kf_mp"][K]), 3)
    conn = H.covis_update(K)
    return dict(tgt_kf=np.array(targets, np.int32), n_cand=len(cand), conn=conn, **{k: np.array(v, np.int32) for k, v in counts.items()})


def m_ba(H, K):
    r = H.P.ba(H, K)
    H.m["mp_pos"], H.ba["kf_pose"], H.ba["kf_twc"], H.ba["mp_assoc"] = r["mp_pos"], r["kf_pose"], r["kf_twc"], r["mp_assoc"]
    H.erase, H.win_mp = np.asarray(r["erase_obs"], np.int32), np.asarray(r["win_mp"], np.int32)
    H.events["ba_erased"] += len(H.erase)
    return dict(sizes=np.asarray(r["sizes"], np.int32), erase_obs=H.erase, win_mp=H.win_mp)


def m_erase(H, K):
    M = H.model()
    M.ba_erase(H.erase)
    rows = E.Model.to_rows(M)
    H.take(M, rows)
    H.events["dead_by_erase"] += len(M.dead)
    return dict(dead_mp=rows["dead_mp"], nobs=H.sizes[2])


def m_refresh_window(H, K):
    H.P.refresh(H, held_valid(H, H.win_mp), 2)
    return {}


def m_remove_key_frames(H, K):
    c = R.connections_vec(H.m, K)
    conn = c["conn_kf"][:CCAP]
    stored = H.G.best_covisibles(K, 0)[0]
    H.events["stale_cull_list"] += list(stored)[:CCAP] != conn.tolist()
    M = H.model()
    cull = M.remove_key_frames(conn, H.kf_depth[:H.sizes[1]], SS.TH_DEPTH)
    rows = E.Model.to_rows(M)
    H.take(M, rows)
    gone = cull["cull_rows"]
    for r in gone:
        H.G.remove_key_frame(int(r), H.ba["kf_first"])
    res = CR.rows_remove(H.g, H.sizes[1], gone.tolist(), H.ba["kf_first"])
    H.graph_agrees(("remove", K))
    H.events["kf_culled"] += len(gone)
    H.events["dead_by_cull"] += len(M.dead)
    return dict(conn_kf=conn, n_conn=len(c["conn_kf"]), cull=cull["cull"], num_mps=cull["num_mps"], num_redundant=cull["num_redundant"],
                cand_status=cull["status"], cull_rows=gone, dead_mp=rows["dead_mp"], nobs=H.sizes[2], covis_result=res)


MODEL_STEPS = (m_track, m_bow, m_add, m_candidates, m_refresh_row, m_covis, m_remove_points, m_create_points, m_search_in_neighbours, m_ba, m_erase,
               m_refresh_window, m_remove_key_frames)


def model_leg(sc, P, check=None):
    """-> (per (K, step) the snapshot and the step's results, the Host).  check(snapshot, K, step) is called after every step."""
    H = Host(sc, P)
    out = collections.OrderedDict()
    entry = H.snapshot()
    for K in sc["arrivals"]:
        arrive(H, K)
        for name, fn in zip(STEPS, MODEL_STEPS):
            res = fn(H, K)
            snap = H.snapshot()
            if check is not None:
                check(snap, K, name)
            out[(K, name)] = (snap, res)
    tr = H.nobs_trace
    low = np.minimum.accumulate(tr)
    H.events["nobs_shrinks_and_grows_again"] += int(any(tr[i] > low[i] and low[i] < tr[0] for i in range(len(tr))))
    return out, H, entry


EVENTS = ("walk_attached", "walk_already", "mp_removed", "kept_met_again", "created", "created_at_two_neighbours", "created_feature_is_no_query_later",
          "fuse_attached", "fuse_replaced", "arrival_followed_replaced", "ba_erased", "dead_by_erase", "kf_culled", "targets_after_a_cull",
          "nobs_shrinks_and_grows_again")
# what the CPU session (the oracle's floats) reached of the events that floats decide; tests/test_session_ref.py asserts these, the GPU
# session each of them halved and at least 1
CPU_REACHED = dict(created=30, created_feature_is_no_query_later=23, fuse_attached=31, fuse_replaced=16, ba_erased=2, dead_by_erase=1, kf_culled=2)


def events_of_results(out):
    """the session's events counted from the step results alone (either leg's, on the host) -> Counter"""
    ev = collections.Counter()
    nobs, culled = [], 0
    for (K, name), (snap, r) in out.items():
        nobs.append(int(snap["sizes"][2]))
        if name == "1b add":
            ev["walk_attached"] += int(r["n_attached"])
            ev["walk_already"] += int(r["n_already"])
        elif name == "2 remove points":
            ev["mp_removed"] += int(np.asarray(r["result"])[1])
        elif name == "3 create points":
            made = np.asarray(r["nb_stats"])[:, 3]
            searched = np.nonzero(np.asarray(r["nb_stats"])[:, 1] == 0)[0]
            ev["created"] += int(r["n_new"])
            ev["created_at_two_neighbours"] += int((made > 0).sum() >= 2)
            ev["created_feature_is_no_query_later"] += int(sum(made[j] for j in searched[:-1]))
        elif name == "4 search in neighbours":
            ev["fuse_attached"] += int(np.sum(r["n_attached"]))
            ev["fuse_replaced"] += int(np.sum(r["n_replaced"]))
            ev["targets_after_a_cull"] += int(culled > 0 and len(r["tgt_kf"]) > 0)
        elif name == "5a ba":
            ev["ba_erased"] += len(r["erase_obs"])
        elif name == "5c erase":
            ev["dead_by_erase"] += len(r["dead_mp"])
        elif name == "6 remove key-frames":
            culled += len(r["cull_rows"])
            ev["kf_culled"] += len(r["cull_rows"])
    low = np.minimum.accumulate(nobs)
    ev["nobs_shrinks_and_grows_again"] += int(any(nobs[i] > low[i] and low[i] < nobs[0] for i in range(len(nobs))))
    return ev


# ---------------------------------------------------------------------------------------------------------------- the invariants
def check_state(s, step=None):
    """What holds of the resident map after EVERY step of the session, said in numpy alone (no model): `s` is a snapshot - the arrays cut
    to the sizes.  tests/test_session_ref.py shows that the models hold each of these after every step.
    Kept: obs_ptr is a row pointer that ends at NOBS; every CSR entry's slot holds its point and no point observes a key-frame twice; an
    invalid point has no entry and no entry names an invalid key-frame; mp_ref_kf of a valid point with entries observes it; found <=
    visible (every rule adds to visible whenever it adds to found: tracking.cpp:222 / :283, map.cpp:142-143, mappoint.cpp:19); the
    candidates are rows of the map; mp_replaced ends at a row that was not replaced; every graph row is weight-descending with ties to
    the lowest row, its ordered prefix the whole row or the prefix rule of covis_ref, the row of an invalid key-frame empty, best_cov -1
    or a row.
    NOT kept, because the reference legitimately breaks them:
      - `no row names a culled key-frame`: Map::removeKeyFrame erases the key-frame from the rows ITS OWN weight map names (map.cpp:
        77-80); a row that names it with a weight below 15 was never told to it (keyframe.cpp:283-296) and goes on naming it, and the
        next addConnection into that row sorts it into the ordered list (:130-150) - the readers test not_valid_ (localization.cpp:162,
        :172);
      - symmetric weights: only a key-frame's own updateConnections rewrites its row, the other rows keep the weight they were told last
        (keyframe.cpp:116-128);
      - `every slot names a valid point that observes the key-frame`: a culled key-frame keeps its mappoints_ (map.cpp:70-76) and a row
        handed over by the tracking thread may hold a point that died since; only the CSR -> slot direction is an invariant."""
    NMP, NKF, NOBS = (int(v) for v in s["sizes"])
    NFK = s["kf_mp"].shape[1]
    ptr, okf, ofeat = s["obs_ptr"].astype(np.int64), s["obs_kf"].astype(np.int64), s["obs_feat"].astype(np.int64)
    assert len(ptr) == NMP + 1 and len(okf) == NOBS == len(ofeat) and s["kf_mp"].shape[0] == NKF == len(s["kf_valid"]), (step, "shapes")
    assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] == NOBS, (step, "obs_ptr is not a CSR row pointer ending at NOBS")
    owner = np.repeat(np.arange(NMP), np.diff(ptr))
    assert ((okf >= 0) & (okf < NKF) & (ofeat >= 0) & (ofeat < NFK)).all(), (step, "an entry outside the tables")
    assert (s["kf_mp"][okf, ofeat] == owner).all(), (step, "a CSR entry whose slot does not hold the point", owner[s["kf_mp"][okf, ofeat] != owner][:5])
    pair = owner * NKF + okf
    assert len(np.unique(pair)) == len(pair), (step, "a point observes a key-frame twice")
    assert (np.diff(ptr)[s["mp_valid"] == 0] == 0).all(), (step, "an invalid point with entries")
    assert (s["kf_valid"][okf] != 0).all(), (step, "an entry names an invalid key-frame")
    has = (s["mp_valid"] != 0) & (np.diff(ptr) > 0)
    ref = s["mp_ref_kf"].astype(np.int64)
    obs_ref = np.zeros(NMP, bool)
    obs_ref[owner[okf == ref[owner]]] = True
    assert obs_ref[has].all(), (step, "mp_ref_kf of a valid point with entries does not observe it", np.nonzero(has & ~obs_ref)[0][:5])
    assert (s["found"][:NMP] <= s["visible"][:NMP]).all(), (step, "found > visible")
    c = s["cand"].astype(np.int64)
    assert ((c >= 0) & (c < NMP)).all(), (step, "a candidate outside the map")
    rep = s["mp_replaced"].astype(np.int64)
    assert ((rep >= -1) & (rep < NMP)).all(), (step, "mp_replaced outside the map")
    at = np.arange(NMP)
    for _ in range(NMP + 1):
        nxt = np.where(rep[at] >= 0, rep[at], at)
        if (nxt == at).all():
            break
        at = nxt
    assert (rep[at] == -1).all(), (step, "mp_replaced does not end")
    W = s["cov_kf"].shape[1]
    n, nord = s["cov_n"].astype(np.int64), s["cov_nord"].astype(np.int64)
    assert ((n >= 0) & (n <= W) & (nord >= 0) & (nord <= n)).all(), (step, "graph lengths")
    assert (n[NKF:] == 0).all() and (n[:NKF][s["kf_valid"] == 0] == 0).all(), (step, "a row of an invalid key-frame is not empty")
    bc = s["best_cov"]
    assert ((bc == -1) | ((bc >= 0) & (bc < NKF))).all(), (step, "best_cov")
    for k in range(NKF):
        kk, ww = s["cov_kf"][k, :n[k]].astype(np.int64), s["cov_w"][k, :n[k]].astype(np.int64)
        assert ((kk >= 0) & (kk < NKF) & (kk != k)).all() and len(np.unique(kk)) == len(kk), (step, k, "graph row names")
        assert (ww > 0).all(), (step, k, "a weight of zero")
        o = np.lexsort((kk, -ww))
        assert (o == np.arange(len(kk))).all(), (step, k, "a row is not weight-descending with ties to the lowest row")
        strong = max(int((ww >= CR.TH).sum()), 1) if n[k] else 0
        assert nord[k] in (n[k], strong), (step, k, "cov_nord is neither the whole row nor the prefix rule", int(nord[k]), int(n[k]), strong)


# ---------------------------------------------------------------------------------------------------------------- CPU float producers
class OracleProducers:
    """the float producers on the CPU: the C++ oracle (fuse search, projection, searchForTriangulation, the createMapPoints block, the
    joint optimisation, renderView + searchCorrespondence) and the numpy restatements (the window, the write-back, update_map_points)"""

    def __init__(self, oracle, cam, mean, cov):
        self.o, self.cam = oracle, cam
        self.h = oracle.gmm_create(mean, np.asarray(cov).reshape(-1, 9))

    def close(self):
        self.o.gmm_destroy(self.h)

    def search2d(self, pose, uv, k):
        out = [(self.o.render_view(self.h, self.cam, pose[b]), self.o.search_correspondence(self.h, uv[b], k))[1] for b in range(len(pose))]
        return np.stack([c for c, _ in out]), np.stack([n for _, n in out])

    def refresh(self, H, mask, what):
        NKF = H.sizes[1]
        out = dict(desc=H.m["mp_desc"], normal=H.m["mp_normal"], max_dist=H.m["mp_max_dist"], min_dist=H.m["mp_min_dist"])
        MP.update_map_points_ref(dict(twc=H.ba["kf_twc"], valid=H.m["kf_valid"], oct=H.ba["kf_oct"], desc=H.kt["desc"][:NKF]),
                                 dict(pos=H.m["mp_pos"], valid=np.asarray(mask, np.uint8), ref_kf=H.ref, obs_ptr=H.m["obs_ptr"], obs_kf=H.m["obs_kf"],
                                      obs_feat=H.ba["obs_feat"]), out, what=what)

    def fuse_best(self, H, kf, cand):
        NMP = H.sizes[0]
        c = cand.astype(np.int64)
        inside = (c >= 0) & (c < NMP)
        c = np.where(inside, c, 0)
        flag = (inside & (H.m["mp_valid"][c] != 0)).astype(np.uint8)
        uvr, level, _, _, inview, _ = self.o.project_map_points(self.cam, H.ba["kf_pose"][kf], H.ba["kf_twc"][kf], H.m["mp_pos"][c], H.m["mp_normal"][c],
                                                                H.m["mp_max_dist"][c], H.m["mp_min_dist"][c], flag)
        feat = H.ba["kf_uvr"][kf]
        bi, _, _ = self.o.fuse_search(self.cam.width, self.cam.height, feat[:, :2], feat[:, 2].astype(f32), H.ba["kf_oct"][kf], H.kt["desc"][kf], uvr, level,
                                      inview, H.m["mp_desc"][c])
        return bi

    def create(self, H, K, conn, n_conn):
        from tests import keyframe_cases as kc
        search = lambda kf1, kf2, fmat, epi: self.o.search_for_triangulation(kf1, kf2, fmat, epi, only_stereo=False, check_orientation=False)[0]
        create = lambda **a: self.o.create_map_points(self.h, self.cam, *[a[k] for k in kc.CMP_KEYS])
        return CP.create_points(self.cam, H.m, H.ba, H.kt_view(), K, conn, n_conn, 0, NN, default_mb(self.cam), H.sizes[0], search, create)

    def ba(self, H, K):
        slab, wins = R.ba_window_build(H.m, H.ba, [K], S.empty_slab(1, BA_CAPS))
        P, F, L, nobs = (int(v) for v in slab["sizes"][0])
        assert not int(slab["status"][0]) & (R.P_TRUNC | R.F_TRUNC | R.L_TRUNC | R.O_TRUNC | R.BAD_ROW)
        dropped, erase = np.zeros((1, BA_CAPS[2]), np.uint8), np.zeros((1, BA_CAPS[3]), np.uint8)
        it = 0
        if L > 0 and nobs > 0:
            poses, points, d, e, it = self.o.joint_optimization(self.h, self.cam, P, F, slab["poses"][0, :P + F], slab["prior"][0, :P], slab["points"][0, :L],
                                                                slab["assoc"][0, :L], slab["obs_ptr"][0, :L + 1], slab["obs_pose"][0, :nobs],
                                                                slab["obs_uvr"][0, :nobs], slab["obs_oct"][0, :nobs])
            slab["poses"][0, :P + F], slab["points"][0, :L], dropped[0, :L], erase[0, :nobs] = poses, points, d, e
        rows, lists = R.ba_window_apply(dict(kf_pose=H.ba["kf_pose"], kf_twc=H.ba["kf_twc"], mp_pos=H.m["mp_pos"], mp_assoc=H.ba["mp_assoc"]), slab,
                                        dropped, erase, np.array([int(it)]))
        return dict(rows, erase_obs=lists[0], win_mp=slab["win_mp"][0, :L].copy(), sizes=(P, F, L, nobs))


# ---------------------------------------------------------------------------------------------------------------- device float producers
class DeviceProducers:
    """the float producers on the device, each on the host's map uploaded afresh (exact sizes, nothing resident between two calls)"""

    def __init__(self, torch, ctx, cam, mean, cov):
        from gmmloc_amd import api
        self.torch, self.ctx, self.cam, self.prm = torch, ctx, cam, api.Params()
        self.gmm = api.GMM(ctx, mean, cov)

    def T(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def search2d(self, pose, uv, k):
        cand, ncand, _, _ = self.gmm.search2d(self.cam, self.T(pose), self.T(uv), k=k)
        return cand.cpu().numpy(), ncand.cpu().numpy()

    def upload(self, H, extra_obs=0):
        md = {k: self.T(v) for k, v in H.m.items()}
        bd = {k: self.T(v) for k, v in H.ba.items() if k != "kf_first"}
        if extra_obs:
            pad = np.zeros(extra_obs, np.int32)
            md["obs_kf"], bd["obs_feat"] = self.T(np.concatenate([H.m["obs_kf"], pad])), self.T(np.concatenate([H.ba["obs_feat"], pad]))
        bd["kf_first"] = H.ba["kf_first"]
        return md, bd, self.T(H.ref), {k: self.T(v) for k, v in H.kt_view().items()}

    def refresh(self, H, mask, what):
        from gmmloc_amd import covis
        md, bd, rk, kt = self.upload(H)
        rows = self.T(np.nonzero(mask)[0].astype(np.int32))
        if rows.shape[0]:
            covis.refresh_points(self.ctx, md, bd, kt, rk, H.sizes, rows, what)
        for k, _, _ in POINT_SPEC:
            H.m[k] = md[k].cpu().numpy()

    def fuse_best(self, H, kf, cand):
        from gmmloc_amd import map_grow
        md, bd, _, kt = self.upload(H, extra_obs=len(cand))
        r = map_grow.fuse_observations_from_map(self.ctx, self.cam, md, bd, kt, kf, self.T(cand), sizes=H.sizes)
        assert r["status"] == 0
        return r["best_idx"].cpu().numpy()

    def create(self, H, K, conn, n_conn):
        from gmmloc_amd import map_grow
        md, bd, _, kt = self.upload(H)
        o = map_grow.create_map_points_on_map(self.ctx, self.gmm, self.cam, self.prm, {k: md[k] for k in CSR_KEYS}, {k: bd[k] for k in SS.BA_ROW_KEYS}, kt, K,
                                              self.T(conn), self.T(np.array([n_conn], np.int32)), first_nb=0, n_nb=NN, mp_base=H.sizes[0])
        s = {k: v.cpu().numpy() for k, v in o.items()}
        s["n_new"] = int(s["n_new"][0])
        return s

    def ba(self, H, K):
        from gmmloc_amd import api
        md, bd, _, _ = self.upload(H)
        r = api.joint_optimization_from_map(self.ctx, self.gmm, self.cam, self.prm, md, bd, K, BA_CAPS)
        return dict(kf_pose=bd["kf_pose"].cpu().numpy(), kf_twc=bd["kf_twc"].cpu().numpy(), mp_pos=md["mp_pos"].cpu().numpy(), mp_assoc=bd["mp_assoc"].cpu().numpy(),
                    erase_obs=r["erase_obs"].cpu().numpy(), win_mp=r["win_mp"].cpu().numpy(), sizes=(r["P"], r["F"], r["L"], r["nobs"]))


# ---------------------------------------------------------------------------------------------------------------- the device leg
GUARD = 64
SENTINEL = {"uint8": 0xA5, "int32": -77, "float32": -7777.0, "float64": -7777.0}
KT_FILL = {"kf_mp": -1}


class Device:
    """ONE set of capacity buffers - NMPcap / OBScap / Wcap / the candidate capacity of `caps`, the key-frame tables at the scene's NKF
    rows -, GUARD sentinel words behind each, filled once from the model leg's state on entry; after that nothing is uploaded but each
    key-frame's own rows (d_arrive) and the tracked frame of step 0"""

    def __init__(self, torch, ctx, sc, entry, caps, cam, gmm, voc):
        from gmmloc_amd import api
        self.torch, self.ctx, self.sc, self.cam, self.gmm, self.voc, self.prm = torch, ctx, sc, cam, gmm, voc, api.Params()
        self.NMPcap, self.OBScap, self.Wcap, self.cand_cap = caps
        self.full = {}
        NKF, NFK = sc["NKF"], sc["NFK"]
        e = entry
        mp, ob = self.NMPcap, self.OBScap
        b = self.buffer
        self.md = dict(mp_valid=b("mp_valid", e["mp_valid"], mp), kf_valid=b("kf_valid", e["kf_valid"], NKF), kf_mp=b("kf_mp", e["kf_mp"], NKF, -1),
                       obs_ptr=b("obs_ptr", e["obs_ptr"], mp + 1), obs_kf=b("obs_kf", e["obs_kf"], ob), mp_pos=b("mp_pos", e["mp_pos"], mp))
        for k, _, _ in POINT_SPEC:
            self.md[k] = b(k, e[k], mp)
        self.bd = {k: b(k, e[k], NKF) for k in SS.BA_ROW_KEYS}
        self.bd.update(obs_feat=b("obs_feat", e["obs_feat"], ob), mp_assoc=b("mp_assoc", e["mp_assoc"], mp), kf_first=int(sc["ba"]["kf_first"]))
        self.rk = b("mp_ref_kf", e["mp_ref_kf"], mp)
        self.st = dict(visible=b("visible", e["visible"], mp), found=b("found", e["found"], mp), ref_idx=b("ref_idx", e["ref_idx"], mp, -1), kf_idx=None,
                       cand=b("cand", e["cand"], self.cand_cap), n_cand=b("n_cand", np.array([len(e["cand"])], np.int32), 1))
        self.rep = b("mp_replaced", e["mp_replaced"], mp, -1)
        W = self.Wcap
        assert int(e["cov_n"].max()) <= W
        self.cov = dict(cov_kf=b("cov_kf", e["cov_kf"][:, :W], NKF), cov_w=b("cov_w", e["cov_w"][:, :W], NKF), cov_n=b("cov_n", e["cov_n"], NKF),
                        cov_nord=b("cov_nord", e["cov_nord"], NKF), best_cov=b("best_cov", e["best_cov"], NKF))
        self.kt = {k: b("kt_" + k, v, NKF) for k, v in sc["kt"].items()}
        self.kt.update({k: b("kt_" + k, e["kt_" + k], NKF) for k in FV_KEYS})
        self.kf_depth = b("kf_depth", sc["kf_depth"], NKF, -1.0)
        self.sizes = tuple(int(v) for v in e["sizes"])
        self.slab = self.lists = None
        self.status = []  # (what, a device tensor that must be all zero) - read after the last step

    def buffer(self, name, a, rows, fill=0):
        """`a` in a buffer of `rows` rows (the rest `fill`) with GUARD sentinel words behind it -> the view a call gets"""
        a = np.ascontiguousarray(a)
        assert len(a) <= rows, (name, len(a), rows)
        n = rows * int(np.prod(a.shape[1:], dtype=np.int64))
        whole = np.full(n + GUARD, SENTINEL[str(a.dtype)], a.dtype)
        body = whole[:n].reshape((rows,) + a.shape[1:])
        body[...] = fill
        body[:len(a)] = a
        t = self.torch.from_numpy(whole).cuda()
        self.full[name] = (t, n)
        return t[:n].view((rows,) + a.shape[1:])

    def guards_untouched(self):
        for name, (t, n) in self.full.items():
            g = t[n:].cpu().numpy()
            assert (g == np.array(SENTINEL[str(g.dtype)], g.dtype)).all(), "written behind %s" % name

    def T(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def views(self):
        from gmmloc_amd import map_grow
        return map_grow.map_views(self.md, self.bd, self.sizes)

    def snapshot(self):
        """device clones of everything the legs are compared on; the sizes are the host's (the composites' own reads)"""
        s = {k: v.clone() for k, v in self.md.items()}
        s.update({k: v.clone() for k, v in self.bd.items() if k != "kf_first"})
        s.update(mp_ref_kf=self.rk.clone(), visible=self.st["visible"].clone(), found=self.st["found"].clone(), ref_idx=self.st["ref_idx"].clone(),
                 cand=self.st["cand"].clone(), n_cand=self.st["n_cand"].clone(), mp_replaced=self.rep.clone())
        s.update({k: v.clone() for k, v in self.cov.items()})
        s.update({"kt_" + k: self.kt[k].clone() for k in FV_KEYS})
        s["sizes"] = self.sizes
        return s


def snapshot_to_host(s):
    """a Device.snapshot() as Host.snapshot() has it: numpy, every table cut to the sizes"""
    NMP, NKF, NOBS = s["sizes"]
    h = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in s.items()}
    out = dict(sizes=np.array(s["sizes"], np.int32))
    for k in ("mp_valid", "mp_pos", "mp_assoc", "mp_ref_kf", "visible", "found", "ref_idx", "mp_replaced") + tuple(k for k, _, _ in POINT_SPEC):
        out[k] = h[k][:NMP]
    for k in ("kf_valid", "kf_mp") + SS.BA_ROW_KEYS:
        out[k] = h[k][:NKF]
    out.update(obs_ptr=h["obs_ptr"][:NMP + 1], obs_kf=h["obs_kf"][:NOBS], obs_feat=h["obs_feat"][:NOBS], cand=h["cand"][:int(h["n_cand"][0])])
    out.update({k: h[k] for k in GRAPH_KEYS})
    out.update({"kt_" + k: h["kt_" + k] for k in FV_KEYS})
    return out


def d_arrive(D, K):
    torch = D.torch
    row = D.sc["rows"][K]
    NMP, NKF, NOBS = D.sizes
    assert NKF == K
    held = D.T(row["kf_mp"]).long()
    ok = (held >= 0) & (held < NMP)
    to = torch.where(ok, D.rep[torch.where(ok, held, torch.zeros_like(held))].long(), torch.full_like(held, -1))
    D.md["kf_mp"][K].copy_(torch.where(to >= 0, to, held).int())
    D.md["kf_valid"][K] = 0
    for key in SS.BA_ROW_KEYS:
        D.bd[key][K].copy_(D.T(row[key]))
    for key in SS.KT_ROW_KEYS:
        D.kt[key][K].copy_(D.T(row[key]))
    D.kf_depth[K].copy_(D.T(row["kf_depth"]))
    D.sizes = (NMP, K + 1, NOBS)
    D.row = torch.full((1,), K, dtype=torch.int32, device="cuda")


def d_track(D, K, inputs):
    from gmmloc_amd import map_stats
    a = {k: D.T(v) for k, v in inputs.items()}
    map_stats.map_stats_track(D.ctx, D.st, D.sizes[0], a["feat_mp"], a["match_local"], a["outlier"], a["inview"], a["local_mp"], a["n_local_mp"])
    return {}


def d_bow(D, K, _=None):
    from gmmloc_amd import bow
    D.status.append((("bow", K), bow.transform_into_tables(D.ctx, D.voc, D.kt, K)))
    return {}


def d_add(D, K, _=None):
    from gmmloc_amd import map_grow
    r = map_grow.map_add(D.ctx, D.md, D.bd, D.sizes, new_kf=D.row, walk_kf=D.row, mp_ref_kf=D.rk)
    D.sizes, D.already = r["sizes"], r["already_mp"]
    return dict(n_attached=r["n_attached"], n_skipped=r["n_skipped"], n_already=r["n_already"], status=r["status"], already_mp=r["already_mp"])


def d_candidates(D, K, _=None):
    from gmmloc_amd import map_stats
    if D.already.shape[0]:
        D.status.append((("cand_append", K), map_stats.map_cand_append(D.ctx, D.st, rows=D.already.contiguous())[1:]))
    return {}


def d_refresh_row(D, K, _=None):
    from gmmloc_amd import covis
    covis.refresh_points(D.ctx, D.md, D.bd, D.kt, D.rk, D.sizes, D.md["kf_mp"][K], 3)
    return {}


def d_covis(D, K, _=None):
    from gmmloc_amd import covis
    m1, _ = D.views()
    return covis.covis_update(D.ctx, covis._view(m1), D.cov, K, COV_CCAP)


def d_remove_points(D, K, _=None):
    from gmmloc_amd import map_stats
    m1, b1 = D.views()
    NMP, NKF, NOBS = D.sizes
    r = map_stats.remove_map_points_from_map(D.ctx, m1, b1, D.st, K, mp_ref_kf=D.rk[:NMP])
    D.sizes = (NMP, NKF, r["remove"]["nobs"])
    return dict(verdict=r["cull"]["verdict"], rm_mp=r["cull"]["rm_mp"], result=r["cull"]["result"], dead_mp=r["remove"]["dead_mp"], nobs=r["remove"]["nobs"],
                remove_status=r["remove"]["status"])


def _new_rows(D, K, first, n):
    from gmmloc_amd import map_stats
    if n:
        NKF = D.sizes[1]
        D.status.append((("new_points", K), map_stats.map_stats_new_points(D.ctx, D.st, NKF, first, D.rk[first:first + n].contiguous())))
        D.status.append((("cand_append_new", K), map_stats.map_cand_append(D.ctx, D.st, first=first, n=n)[1:]))


def d_create_points(D, K, _=None):
    from gmmloc_amd import map_grow
    NMP = D.sizes[0]
    r = map_grow.create_map_points_from_map(D.ctx, D.gmm, D.cam, D.prm, D.md, D.bd, D.kt, K, nn=NN, sizes=D.sizes, mp_ref_kf=D.rk)
    D.sizes = r["sizes"]
    _new_rows(D, K, NMP, r["n_new"])
    return dict(n_new=r["n_new"], new_type=r["new_type"], new_nb=r["new_nb"], feat_new=r["feat_new"], nb_stats=r["nb_stats"], n_attached=r["n_attached"],
                n_skipped=r["n_skipped"], status=r["status"])


def d_create_points_split(D, K, _=None):
    """the public per-call route: ONE neighbour per gl_create_map_points_from_map call, map_add between two of them"""
    from gmmloc_amd import api, covis, map_grow
    torch = D.torch
    NMP = D.sizes[0]
    m1, _ = D.views()
    conn = api.update_connections(D.ctx, covis._view(m1), D.row, Ccap=NN)
    att = skipped = 0
    types, nbs, feat_new, stats = [], [], None, []
    for j in range(NN):
        m1, b1 = D.views()
        s = map_grow.create_map_points_on_map(D.ctx, D.gmm, D.cam, D.prm, covis._view(m1), {k: b1[k] for k in SS.BA_ROW_KEYS},
                                              {k: v[:D.sizes[1]] for k, v in D.kt.items()}, K, conn["conn_kf"][0], conn["n_conn"], first_nb=j, n_nb=1,
                                              mp_base=D.sizes[0])
        r = map_grow.map_add(D.ctx, D.md, D.bd, D.sizes, new_mp=dict(pos=s["new_pos"], assoc=s["new_assoc"], ref_kf=s["new_ref_kf"]),
                             attach=dict(mp=s["att_mp"], kf=s["att_kf"], feat=s["att_feat"]), mp_ref_kf=D.rk, n_new_mp=s["n_new"], n_attach=s["n_attach"])
        assert r["status"] == 0
        n = r["sizes"][0] - D.sizes[0]
        D.sizes = r["sizes"]
        att, skipped = att + r["n_attached"], skipped + r["n_skipped"]
        types.append(s["new_type"][:n])
        nbs.append(s["new_nb"][:n])
        stats.append(s["nb_stats"])
        feat_new = s["feat_new"] if feat_new is None else torch.where(s["feat_new"] >= 0, s["feat_new"], feat_new)
    n_new = D.sizes[0] - NMP
    if n_new:
        covis.refresh_points(D.ctx, D.md, D.bd, D.kt, D.rk, D.sizes, torch.arange(NMP, NMP + n_new, dtype=torch.int32, device="cuda"), 3)
    _new_rows(D, K, NMP, n_new)
    return dict(n_new=n_new, new_type=torch.cat(types), new_nb=torch.cat(nbs), feat_new=feat_new, nb_stats=torch.cat(stats), n_attached=att, n_skipped=skipped,
                status=0)


def d_search_in_neighbours(D, K, _=None):
    from gmmloc_amd import covis
    r = covis.search_in_neighbors_from_map(D.ctx, D.cam, D.md, D.bd, D.cov, D.kt, K, K, stats=D.st, mp_replaced=D.rep, mp_ref_kf=D.rk, sizes=D.sizes)
    assert r["status"] == 0, r["status"]
    D.sizes = r["sizes"]
    return dict(tgt_kf=np.array(r["tgt_kf"], np.int32), n_cand=r["n_cand"], conn=r["conn"], n_fused=np.array(r["n_fused"], np.int32),
                n_attached=np.array(r["n_attached"], np.int32), n_replaced=np.array(r["n_replaced"], np.int32))


def d_search_in_neighbours_split(D, K, _=None):
    """the per-call route: the two lists from their own entry points, one fuse_and_note per target, the refresh and the graph update"""
    from gmmloc_amd import covis, map_grow
    NMP, NKF, NOBS = D.sizes
    tg = covis.fuse_targets(D.ctx, D.cov, D.md["kf_valid"], NKF, K, NN, 5)
    head = tg["list"].tolist()
    targets = head[1:1 + head[0]]
    snapshot = D.md["kf_mp"][K].clone()
    counts = dict(n_fused=[], n_attached=[], n_replaced=[])
    def fuse(kf, cand):
        r = covis.fuse_and_note(D.ctx, D.cam, D.md, D.bd, D.kt, kf, cand, D.sizes, D.st, D.rep)
        assert r["status"] == 0
        D.sizes = r["sizes"]
        for k in counts:
            counts[k].append(r[k])
    for t in targets:
        fuse(t, snapshot)
    m1, _ = D.views()
    cd = covis.fuse_candidates(D.ctx, covis._view(m1), tg["tgt_kf"], tg["n_tgt"], K)
    n_cand = int(cd["n_cand"].item())
    fuse(K, cd["cand_mp"][:n_cand].contiguous())
    covis.refresh_points(D.ctx, D.md, D.bd, D.kt, D.rk, D.sizes, D.md["kf_mp"][K], 3)
    m1, _ = D.views()
    conn = covis.covis_update(D.ctx, covis._view(m1), D.cov, K, COV_CCAP)
    return dict(tgt_kf=np.array(targets, np.int32), n_cand=n_cand, conn=conn, **{k: np.array(v, np.int32) for k, v in counts.items()})


def d_search_in_neighbours_host(D, K, _=None):
    """the split route of tests/test_gpu_covis.py: the graph and the two lists in numpy from read-backs, one fuse_observations_from_map
    per target by hand, the refreshes through masks made on the host, the graph uploaded again"""
    from tests.test_gpu_covis import _split_route
    NMP = D.sizes[0]
    s = dict(md=D.md, bd=D.bd, rk=D.rk[:NMP], sizes=D.sizes, kf_desc=D.kt["desc"], cov=D.cov, stats=D.st, rep=D.rep)
    targets, cand, counts, conn = _split_route(D.torch, D.ctx, D.cam, s, K, K)
    for k, v in s["cov"].items():
        D.cov[k].copy_(v)
    D.sizes = s["sizes"]
    return dict(tgt_kf=np.array(targets, np.int32), n_cand=len(cand))


def d_ba(D, K, _=None):
    from gmmloc_amd import api
    m1, b1 = D.views()
    r = api.joint_optimization_from_map(D.ctx, D.gmm, D.cam, D.prm, m1, b1, K, BA_CAPS, slab=D.slab)
    D.slab, D.ba_r = r["slab"], r
    return dict(sizes=np.array([r["P"], r["F"], r["L"], r["nobs"]], np.int32), erase_obs=r["erase_obs"].clone(), win_mp=r["win_mp"].clone())


def d_erase(D, K, _=None):
    from gmmloc_amd import api
    m1, b1 = D.views()
    NMP, NKF, NOBS = D.sizes
    e = api.map_remove(D.ctx, m1, b1, erase_obs=D.slab["erase_obs"][0], n_erase=D.slab["n_erase"], mp_ref_kf=D.rk[:NMP])
    assert e["status"] == 0
    D.sizes = (NMP, NKF, e["nobs"])
    return dict(dead_mp=e["dead_mp"], nobs=e["nobs"])


def d_refresh_window(D, K, _=None):
    from gmmloc_amd import covis
    covis.refresh_points(D.ctx, D.md, D.bd, D.kt, D.rk, D.sizes, D.ba_r["win_mp"], 2)
    return {}


def d_remove_key_frames(D, K, _=None):
    from gmmloc_amd import api, covis
    m1, b1 = D.views()
    NMP, NKF, NOBS = D.sizes
    if D.lists is None:  # the two output dicts a caller may bring, guarded like the capacity buffers and used again for every key-frame
        z = lambda name, dt, fill=0, n=CCAP: D.buffer("out_" + name, np.full((1, n), fill, dt), 1)
        D.lists = (dict(conn_kf=z("conn_kf", np.int32, -1), conn_w=z("conn_w", np.int32), n_conn=z("n_conn", np.int32, 0, 1)[0], status=z("status", np.int32, 0, 1)[0]),
                   dict(cull=z("cull", np.uint8), num_mps=z("num_mps", np.int32), num_redundant=z("num_redundant", np.int32), cand_status=z("cand_status", np.int32),
                        cull_rows=z("cull_rows", np.int32, -1), n_cull=z("n_cull", np.int32, 0, 1)[0]))
    conn = api.update_connections(D.ctx, covis._view(m1), D.row, out=D.lists[0])
    cull = api.cull_keyframes(D.ctx, m1, b1, D.kf_depth[:NKF], SS.TH_DEPTH, conn["conn_kf"], conn["n_conn"], out=D.lists[1])
    conn, cull = {k: v.clone() for k, v in conn.items()}, {k: v.clone() for k, v in cull.items()}  # (the next key-frame writes the same buffers)
    k = api.map_remove(D.ctx, m1, b1, rm_kf=cull["cull_rows"][0], n_rm_kf=cull["n_cull"], mp_ref_kf=D.rk[:NMP])
    assert k["status"] == 0
    res = covis.covis_remove(D.ctx, D.cov, NKF, cull["cull_rows"][0], cull["n_cull"], D.bd["kf_first"])
    D.sizes = (NMP, NKF, k["nobs"])
    return dict(conn_kf=conn["conn_kf"][0], n_conn=conn["n_conn"], cull=cull["cull"][0], num_mps=cull["num_mps"][0], num_redundant=cull["num_redundant"][0],
                cand_status=cull["cand_status"][0], cull_rows=cull["cull_rows"][0], n_cull=cull["n_cull"], dead_mp=k["dead_mp"], nobs=k["nobs"], covis_result=res)


def d_mapping_pass(D, K, _=None):
    """steps 5a .. 6d in the one call a host makes for them: api.mapping_pass_from_map with the key-frame tables and the graph"""
    from gmmloc_amd import api
    m1, b1 = D.views()
    NMP, NKF, NOBS = D.sizes
    p = api.mapping_pass_from_map(D.ctx, D.gmm, D.cam, D.prm, m1, b1, K, BA_CAPS, D.kf_depth[:NKF], SS.TH_DEPTH, Ccap=CCAP, mp_ref_kf=D.rk[:NMP], slab=D.slab,
                                  kf_tables=D.kt, cov=D.cov)
    assert p["status"] == (0, 0)
    D.slab = p["ba"]["slab"]
    D.sizes = (NMP, NKF, p["map"]["obs_kf"].shape[0])
    return dict(culled=p["culled"], erased=p["erased"])


DEVICE_STEPS = (d_track, d_bow, d_add, d_candidates, d_refresh_row, d_covis, d_remove_points, d_create_points, d_search_in_neighbours, d_ba, d_erase,
                d_refresh_window, d_remove_key_frames)
SPLIT = {d_create_points: d_create_points_split, d_search_in_neighbours: d_search_in_neighbours_split}


def device_leg(D, track_inputs, split=False, one_pass=False):
    """every key-frame of the scene on D, nothing read back but what the composites themselves read -> per (K, step) (Device.snapshot(),
    the step's results), every tensor still on the device.  track_inputs: {K: the model leg's inputs of step 0}.  split: the composites
    of steps 3 and 4 replaced by their per-call routes ("host": step 4 by the split route of tests/test_gpu_covis.py, which reads back);
    one_pass: steps 5a .. 6 in ONE api.mapping_pass_from_map call (made at 5a; the
    snapshots of 5c and 5b are then those of the whole pass)."""
    out = collections.OrderedDict()
    for K in D.sc["arrivals"]:
        d_arrive(D, K)
        for name, fn in zip(STEPS, DEVICE_STEPS):
            fn = SPLIT.get(fn, fn) if split else fn
            fn = d_search_in_neighbours_host if split == "host" and fn is d_search_in_neighbours_split else fn
            if one_pass and fn in (d_ba, d_erase, d_refresh_window, d_remove_key_frames):
                fn = d_mapping_pass if fn is d_ba else (lambda D, K: {})
            res = fn(D, K, track_inputs[K]) if fn is d_track else fn(D, K)
            out[(K, name)] = (D.snapshot(), res)
    return out


def results_to_host(name, res):
    """a step's results as numpy / ints (a nested `conn` dict included), the lists cut to the counts the device reports itself"""
    d = {}
    for k, v in res.items():
        d[k] = results_to_host(k, v) if isinstance(v, dict) else v.cpu().numpy() if hasattr(v, "cpu") else v
    if name == "2 remove points":
        kept, removed, erased, _ = (int(v) for v in d["result"])
        d["verdict"], d["rm_mp"] = d["verdict"][:kept + removed + erased], d["rm_mp"][:removed]
        assert d.pop("remove_status") == 0
    if name == "6 remove key-frames" and d:
        n, nc = min(int(d["n_conn"][0]), CCAP), int(d.pop("n_cull")[0])
        for k in ("conn_kf", "cull", "num_mps", "num_redundant", "cand_status"):
            d[k] = d[k][:n]
        d["cull_rows"], d["n_conn"] = d["cull_rows"][:nc], int(d["n_conn"][0])
    return d


def same_results(name, d, ref, what):
    """a step's counts and lists"""
    assert sorted(d) == sorted(k for k in ref if k != "inputs"), (what, sorted(d), sorted(ref))
    for k, v in d.items():
        if isinstance(v, dict):
            same_results(k, v, ref[k], what + (k,))
            continue
        a, b = np.asarray(v), np.asarray(ref[k])
        assert a.shape == b.shape and (a == b).all(), (what, k, a.ravel()[:12].tolist(), b.ravel()[:12].tolist())
