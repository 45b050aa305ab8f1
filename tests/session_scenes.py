"""The scene of the mapping session (tests/session_ref.py): tests/map_grow_scenes.geo_scene with its last T key-frames handed over one at
a time, the key-frame tables createMapPoints reads, counters, a candidate list and the tracked frames of step 0 - everything seeded.
Test infrastructure; nothing in the product imports it.

The knobs (KNOBS) exist so that every event tests/test_session_ref.py asks for happens at least once over the T key-frames:
  n_twins / n_forget  geo_scene's: split points (a fuse replaces) and forgotten observations (a fuse attaches)
  n_latent            points taken OUT of the map whose features stay where they were: unheld features of the arriving key-frames and of
                      their neighbours that look alike and satisfy the epipolar constraint - what createMapPoints triangulates
  n_share             further observations of an arriving key-frame's points by each of the three key-frames before it
  n_dup               held points written into a second slot of an arriving row: the walk meets them a second time (already_mp)
  n_cand0, ratio_low  the candidate list on entry and the share of it with found / visible < 0.25
  oct_max             the octaves clamped as tests/map_edit_scenes.py clamps them, so that key-frames ARE culled
  cullable, depth_min_obs  in the rows `cullable` only the features of points with that many observers keep a depth for the cull (as
                      test_mapping_pass_equals_the_host_edits does): those key-frames are redundant once they are in the list
  track_frac, local_n the subset of the arriving row the tracked frame of step 0 holds, the size of its local map"""
import numpy as np

from gmmloc_amd import api, synth
from tests import map_edit_scenes as ES
from tests import map_grow_scenes as GS

KNOBS = dict(T=4, n_twins=90, n_forget=90, n_latent=70, n_share=9, n_dup=3, n_cand0=160, ratio_low=0.2, oct_max=1, cullable=(17, 19), depth_min_obs=7,
             track_frac=0.7, local_n=200, seed=20, voc=(10, 3, 14), k=5)
TH_DEPTH = ES.TH_DEPTH
KT_ROW_KEYS = ("desc", "angle", "depth", "cand", "ncand")   # a key-frame's own table rows: part of its one upload
BA_ROW_KEYS = ("kf_pose", "kf_twc", "kf_uvr", "kf_oct")


def _remove_points(m, ba, rows):
    """the points `rows` taken out of the map as if they had never been made: invalid, no entry, no slot"""
    NMP = len(m["mp_valid"])
    owner = np.repeat(np.arange(NMP), np.diff(m["obs_ptr"]))
    gone = np.zeros(NMP, bool)
    gone[rows] = True
    keep = ~gone[owner]
    ptr = np.zeros(NMP + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(owner[keep], minlength=NMP))
    kf_mp = m["kf_mp"].copy()
    kf_mp[(kf_mp >= 0) & gone[np.maximum(kf_mp, 0)]] = -1
    mpv = m["mp_valid"].copy()
    mpv[rows] = 0
    return dict(m, mp_valid=mpv, kf_mp=kf_mp, obs_ptr=ptr.astype(np.int32), obs_kf=m["obs_kf"][keep]), dict(ba, obs_feat=ba["obs_feat"][keep])


def _share(m, ba, kf_desc, K, N, n, rng, cam):
    """up to n points that key-frame K holds and key-frame N does not become observations of N too - the feature where the point
    projects, the descriptor of K's feature with six bits flipped, the octave the distance predicts - in N's free slots, then in slots
    whose point nobody else observes (that point is taken out of the map).  Everything IN PLACE on copies the caller made; the CSR is
    rebuilt by _csr_from.  -> the rows taken out"""
    NMP = len(m["mp_valid"])
    on = (m["kf_mp"] >= 0) & (m["kf_valid"] != 0)[:, None]
    nobs = np.bincount(m["kf_mp"][on], minlength=NMP)  # (every observation by a valid key-frame has its slot in this scene)
    in_n = set(m["kf_mp"][N][m["kf_mp"][N] >= 0].tolist())
    T = ba["kf_pose"][N]
    Rn = synth.quat_to_R(T[:4])
    free = [int(f) for f in np.nonzero(m["kf_mp"][N] < 0)[0]]
    lone = [int(f) for f in np.nonzero(m["kf_mp"][N] >= 0)[0] if nobs[m["kf_mp"][N][f]] == 1]
    slots, gone, done = free + lone, [], 0
    for fk in rng.permutation(np.nonzero(m["kf_mp"][K] >= 0)[0]):
        p = int(m["kf_mp"][K][fk])
        if done == n or not slots:
            break
        if not m["mp_valid"][p] or p in in_n:
            continue
        pc = Rn @ m["mp_pos"][p] + T[4:]
        if not 0.3 < pc[2] < 8.0:
            continue
        u, v = cam.fx * pc[0] / pc[2] + cam.cx, cam.fy * pc[1] / pc[2] + cam.cy
        if not (0 <= u < cam.width and 0 <= v < cam.height):
            continue
        f = slots.pop(0)
        if m["kf_mp"][N][f] >= 0:
            gone.append(int(m["kf_mp"][N][f]))
        dk, dn = np.linalg.norm(m["mp_pos"][p] - ba["kf_twc"][K]), np.linalg.norm(m["mp_pos"][p] - ba["kf_twc"][N])
        oc = int(np.clip(np.round(ba["kf_oct"][K][fk] + np.log(dk / dn) / np.log(1.2)), 0, 7))
        sig = 0.3 * 1.2 ** oc
        u, v = u + rng.standard_normal() * sig, v + rng.standard_normal() * sig
        ur = u - cam.bf / pc[2] + rng.standard_normal() * sig * 0.5
        ba["kf_uvr"][N, f] = (u, v, float(np.float32(ur)))
        ba["kf_oct"][N, f] = oc
        d = kf_desc[K, fk].copy()
        bits = rng.choice(256, 6, replace=False)
        d[bits >> 3] ^= (1 << (bits & 7)).astype(np.uint8)
        kf_desc[N, f] = d
        m["kf_mp"][N, f] = p
        in_n.add(p)
        done += 1
    return gone


def _csr_from(m, ba):
    """the CSR of a map whose every observation has its slot, from the kf_mp rows of the valid key-frames: per point its key-frames in row order"""
    NMP = len(m["mp_valid"])
    k, f = np.nonzero((m["kf_mp"] >= 0) & (m["kf_valid"] != 0)[:, None])
    p = m["kf_mp"][k, f]
    o = np.lexsort((k, p))
    ptr = np.zeros(NMP + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(p, minlength=NMP))
    return dict(m, obs_ptr=ptr.astype(np.int32), obs_kf=k[o].astype(np.int32)), dict(ba, obs_feat=f[o].astype(np.int32))


def session_scene(mean, cov, gt, search2d, knobs=None):
    """search2d(kf_pose (NKF,7), uv (NKF,NFK,2), k) -> (cand (NKF,NFK,k) i32, ncand (NKF,NFK) i32): GMM::renderView + searchCorrespondence
    of every key-frame at the pose it was made with (the device's gl_search2d or the oracle's).
    -> dict(m, ba, ref: the map on entry, NKF0 key-frame rows; rows: per arriving key-frame its own rows (kf_mp, BA_ROW_KEYS, KT_ROW_KEYS);
    kt: the tables of the NKF0 rows; stats: visible / found / ref_idx / cand on entry; track: per arriving key-frame the seeds of step 0;
    arrivals, NKF, NFK, voc, knobs)"""
    kn = dict(KNOBS, **(knobs or {}))
    sc = GS.geo_scene(mean, cov, gt, n_twins=kn["n_twins"], n_forget=kn["n_forget"])
    m, ba, kf_desc = sc["m"], sc["ba"], sc["kf_desc"]
    rng = np.random.default_rng(kn["seed"])
    NKF, NFK = m["kf_mp"].shape
    arrivals = [int(k) for k in range(NKF - kn["T"], NKF)]
    assert all(m["kf_valid"][k] for k in arrivals)
    # the map as the reference's removals leave one: an invalid point holds nothing and no slot, an invalid key-frame is observed by nobody
    m, ba = _remove_points(m, ba, np.nonzero(m["mp_valid"] == 0)[0])
    for k in np.nonzero(m["kf_valid"] == 0)[0]:
        m, ba = GS.strip_key_frame(m, ba, int(k))
    # more shared points between every arriving key-frame and the three before it: two or more neighbours reach the weight of 15
    m = dict(m, kf_mp=m["kf_mp"].copy())
    ba = dict(ba, kf_uvr=ba["kf_uvr"].copy(), kf_oct=ba["kf_oct"].copy())
    kf_desc = kf_desc.copy()
    gone = []
    for k in arrivals:
        for nb in (k - 1, k - 2, k - 3):
            if m["kf_valid"][nb]:
                gone += _share(m, ba, kf_desc, k, nb, kn["n_share"], rng, api.Camera())
    m, ba = _csr_from(m, ba)
    m, ba = _remove_points(m, ba, np.array(sorted(set(gone)), np.int64))
    ba = dict(ba, kf_oct=np.minimum(ba["kf_oct"], kn["oct_max"]).astype(np.int32))
    # the key-frame tables
    cam = api.Camera()
    uvr = ba["kf_uvr"]
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(uvr[:, :, 2] >= 0, cam.bf / np.maximum(uvr[:, :, 0] - uvr[:, :, 2], 1e-6), -1.0).astype(np.float32)
    NMP = len(m["mp_valid"])
    angle_mp = rng.uniform(0, 360, NMP)
    angle = rng.uniform(0, 360, (NKF, NFK))
    held = m["kf_mp"] >= 0
    angle[held] = (angle_mp[m["kf_mp"][held]] + rng.standard_normal(int(held.sum()))) % 360.0
    cand, ncand = search2d(ba["kf_pose"], np.ascontiguousarray(uvr[:, :, :2]), kn["k"])
    kt = dict(desc=kf_desc, angle=angle.astype(np.float32), depth=depth, cand=np.asarray(cand, np.int32), ncand=np.asarray(ncand, np.int32))
    # the depths the key-frame cull reads: of well-observed points only, so that key-frames are culled on a scene this small
    nobs = np.diff(m["obs_ptr"])
    kf_depth = depth.copy()
    thin = ~held | (nobs[np.maximum(m["kf_mp"], 0)] < kn["depth_min_obs"])
    for k in kn["cullable"]:
        kf_depth[k][thin[k]] = -1.0
    # latent points: stereo in an arriving key-frame, seen by two or more of the others
    ptr = m["obs_ptr"]
    latent = []
    for p in rng.permutation(NMP):
        ks = m["obs_kf"][ptr[p]:ptr[p + 1]]
        fs = ba["obs_feat"][ptr[p]:ptr[p + 1]]
        arr = [(k, f) for k, f in zip(ks, fs) if k in arrivals]
        if m["mp_valid"][p] and len(ks) >= 3 and arr and uvr[arr[0][0], arr[0][1], 2] >= 0 and len(ks) - len(arr) >= 1:
            latent.append(int(p))
        if len(latent) == kn["n_latent"]:
            break
    latent_slot = np.zeros((NKF, NFK), bool)
    for p in latent:
        latent_slot[m["obs_kf"][ptr[p]:ptr[p + 1]], ba["obs_feat"][ptr[p]:ptr[p + 1]]] = True
    m, ba = _remove_points(m, ba, np.array(latent, np.int64))
    # a second slot for a few held points of every arriving row
    kf_mp = m["kf_mp"].copy()
    for k in arrivals:
        free = np.nonzero((kf_mp[k] < 0) & ~latent_slot[k])[0]
        own = kf_mp[k][(kf_mp[k] >= 0) & (m["mp_valid"][np.maximum(kf_mp[k], 0)] != 0)]
        n = min(kn["n_dup"], len(free), len(own))
        kf_mp[k, rng.choice(free, n, replace=False)] = rng.choice(own, n, replace=False)
    m = dict(m, kf_mp=kf_mp)
    for k in arrivals:
        m, ba = GS.strip_key_frame(m, ba, k)
    # a point nobody observes any more was made by the tracking thread at the first arriving key-frame that holds it
    ref = ES.first_entry_kf(m)
    for k in reversed(arrivals):
        p = m["kf_mp"][k]
        p = p[p >= 0]
        p = p[np.diff(m["obs_ptr"])[p] == 0]
        ref[p] = k
    NKF0 = arrivals[0]
    rows = {k: dict(kf_mp=m["kf_mp"][k].copy(), **{key: ba[key][k].copy() for key in BA_ROW_KEYS}, **{key: kt[key][k].copy() for key in KT_ROW_KEYS},
                    kf_depth=kf_depth[k].copy()) for k in arrivals}
    m0 = dict(m, kf_mp=m["kf_mp"][:NKF0].copy(), kf_valid=m["kf_valid"][:NKF0].copy())
    ba0 = dict(ba, **{key: ba[key][:NKF0].copy() for key in BA_ROW_KEYS})
    assert (m0["obs_kf"] < NKF0).all()
    # counters and the candidate list on entry
    alive = np.nonzero((m0["mp_valid"] != 0) & (np.diff(m0["obs_ptr"]) > 0))[0]
    visible = rng.integers(4, 40, NMP).astype(np.int32)
    found = np.minimum(visible, rng.integers(2, 40, NMP)).astype(np.int32)
    found = np.maximum(found, (visible + 1) // 2).astype(np.int32)
    ref_idx = np.where(ref >= 0, ref, -1).astype(np.int32)
    cand0 = rng.choice(alive, min(kn["n_cand0"], len(alive)), replace=False).astype(np.int32)
    low = cand0[rng.uniform(size=len(cand0)) < kn["ratio_low"]]
    found[low] = visible[low] // 5
    ref_idx[cand0] = rng.integers(NKF0 - 2, NKF0 + 1, len(cand0))
    track = {k: int(rng.integers(1 << 30)) for k in arrivals}
    return dict(m=m0, ba=ba0, ref=ref, rows=rows, kt={key: v[:NKF0].copy() for key, v in kt.items()}, kf_depth=kf_depth[:NKF0].copy(),
                stats=dict(visible=visible, found=found, ref_idx=ref_idx, cand=cand0), track=track, arrivals=arrivals, NKF=NKF, NFK=NFK,
                voc=synth.synth_vocabulary(*kn["voc"]), knobs=kn, mean=mean, cov=cov)


def track_inputs(sc, K, m, kf_mp_row):
    """the chain's outputs of the tracked frame that became key-frame K, for gl_map_stats_track / map_stats_ref.model_track: the frame holds
    a seeded subset of the key-frame's own row (valid points only, as the chain leaves them), a tenth of them outliers, and a local map of
    valid points it does not hold, half of them in view"""
    kn = sc["knobs"]
    rng = np.random.default_rng(sc["track"][K])
    NMP = len(m["mp_valid"])
    row = np.asarray(kf_mp_row, np.int32)
    ok = (row >= 0) & (row < NMP)
    ok &= m["mp_valid"][np.where(ok, row, 0)] != 0
    feat_mp = np.where(ok & (rng.uniform(size=len(row)) < kn["track_frac"]), row, -1).astype(np.int32)
    others = np.nonzero((m["mp_valid"] != 0) & ~np.isin(np.arange(NMP), feat_mp))[0]
    local = rng.choice(others, min(kn["local_n"], len(others)), replace=False).astype(np.int32)
    return dict(feat_mp=feat_mp[None], match_local=-np.ones((1, len(row)), np.int32), outlier=(rng.uniform(size=(1, len(row))) < 0.1).astype(np.uint8),
                inview=(rng.uniform(size=(1, len(local))) < 0.5).astype(np.uint8), local_mp=local[None], n_local_mp=np.array([len(local)], np.int32))
