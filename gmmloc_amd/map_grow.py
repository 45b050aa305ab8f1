"""Growing the resident map on the device: gl_map_add (new rows, new key-frames, attach triples, the walk of processNewKeyFrame) and
gl_map_fuse (the second half of fuseObservations with Map::replaceMapPoint); rules in include/gmmloc_hip.h.

The arrays keep their allocation and the counts grow.  `map` / `ba` are the dicts of api.map_remove whose tensors are the CAPACITY
buffers - each table's leading dimension at its capacity instead of its extent (_host.MAP_TABLES: NMPcap for NMP, OBScap for NOBS, at
least NKF key-frame rows) - and `sizes` = (NMP, NKF, NOBS) says how much of them the map fills (None: all of it).  Every call returns the new sizes and
`map` / `ba` cut to them (views of the same tensors): what the readers (api.update_connections, api.ba_window_build, ...) take."""
import ctypes as C

from . import _lib
from ._host import MAP_TABLES, _count, _extents, _map_ba_view, _map_buffers, _map_edit, _map_view, _ptr, _tensor
from .api import fuse_search, project_map_points

GROW_OBS_TRUNCATED, GROW_MP_TRUNCATED, FUSE_REPL_TRUNCATED, ADD_ALREADY_TRUNCATED = 1, 2, 4, 8
_PER_POINT = tuple(k for k, t in MAP_TABLES.items() if t.lead == "NMP" and t.where)  # the tables of NMPcap rows in `map` / `ba`: what a test pads


def map_views(map, ba, sizes):
    """the two dicts cut to sizes = (NMP, NKF, NOBS): views of the same tensors, the dicts the readers of the resident map take - each
    table's leading dimension cut to the extent it follows (_host.MAP_TABLES), anything else as it is"""
    NMP, NKF, NOBS = sizes
    ext = _extents(NMP, NKF, None, NOBS)
    cut = lambda k, t: t[:ext[MAP_TABLES[k].lead]] if k in MAP_TABLES and hasattr(t, "shape") else t
    return {k: cut(k, t) for k, t in map.items()}, {k: cut(k, t) for k, t in ba.items()}


def map_add(ctx, map, ba, sizes=None, new_mp=None, new_kf=None, attach=None, walk_kf=None, mp_ref_kf=None, n_new_mp=None, n_new_kf=None,
            n_attach=None, n_walk=None, already_cap=None, want_new_pos=False):
    """gl_map_add: IN PLACE on the capacity buffers (module docstring).  new_mp: dict(pos (n,3) f64, assoc (n,) i32, ref_kf (n,) i32 -
    needed with mp_ref_kf) - the rows [NMP, NMP + n); needs map['mp_pos'] and ba['mp_assoc'].  new_kf (n,) i32: rows that become valid.
    attach: dict(mp, kf, feat) of (n,) i32, the triples in list order.  walk_kf (n,) i32: the rows whose slots are walked as
    processNewKeyFrame does.  n_x: the length as a 1-element i32 device tensor instead of the tensor's own.  mp_ref_kf (NMPcap,) i32.
    -> dict(sizes (NMP, NKF, NOBS) after the call - the sizes on entry after a truncation, with `needed` = what the call asked for -
    n_attached, n_skipped, n_already, status, already_mp (min(n_already, already_cap),) i32, map, ba: cut to sizes[, obs_new_pos (old
    NOBS,) i32: all -1 after a truncation]).  One 24-byte copy and one synchronise."""
    import torch
    need = ("mp_assoc",) if new_mp is not None else ()
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, need)
    ed = _map_edit(map, ba, mp_ref_kf, NMPcap, dev)
    ls = _lib.gl_map_add_lists()
    if new_mp is not None:
        for k in new_mp:
            assert k in ("pos", "assoc", "ref_kf"), "new_mp[%r]: unknown key" % k
        assert map.get("mp_pos") is not None, "map['mp_pos']: missing"
        n = _tensor("new_mp['pos']", new_mp.get("pos"), "float64", (None, 3), dev).shape[0]
        ls.new_pos, ls.new_mp_cap = _ptr(new_mp["pos"]), n
        ls.new_assoc = _ptr(_tensor("new_mp['assoc']", new_mp.get("assoc"), "int32", (n,), dev))
        if mp_ref_kf is not None or new_mp.get("ref_kf") is not None:
            ls.new_ref_kf = _ptr(_tensor("new_mp['ref_kf']", new_mp.get("ref_kf"), "int32", (n,), dev))
        ls.n_new_mp = _count("n_new_mp", n_new_mp, dev)
    else:
        assert n_new_mp is None, "n_new_mp without new_mp"
    if new_kf is not None:
        ls.new_kf, ls.new_kf_cap = _ptr(_tensor("new_kf", new_kf, "int32", (None,), dev)), new_kf.shape[0]
        ls.n_new_kf = _count("n_new_kf", n_new_kf, dev)
    else:
        assert n_new_kf is None, "n_new_kf without new_kf"
    if attach is not None:
        for k in attach:
            assert k in ("mp", "kf", "feat"), "attach[%r]: unknown key" % k
        n = _tensor("attach['mp']", attach.get("mp"), "int32", (None,), dev).shape[0]
        ls.att_mp, ls.attach_cap = _ptr(attach["mp"]), n
        ls.att_kf = _ptr(_tensor("attach['kf']", attach.get("kf"), "int32", (n,), dev))
        ls.att_feat = _ptr(_tensor("attach['feat']", attach.get("feat"), "int32", (n,), dev))
        ls.n_attach = _count("n_attach", n_attach, dev)
    else:
        assert n_attach is None, "n_attach without attach"
    if walk_kf is not None:
        ls.walk_kf, ls.walk_cap = _ptr(_tensor("walk_kf", walk_kf, "int32", (None,), dev)), walk_kf.shape[0]
        ls.n_walk = _count("n_walk", n_walk, dev)
    else:
        assert n_walk is None, "n_walk without walk_kf"
    already_cap = ls.walk_cap * NFK if already_cap is None else int(already_cap)
    result = torch.zeros(6, dtype=torch.int32, device=dev)
    already = torch.zeros(already_cap, dtype=torch.int32, device=dev)
    new_pos = torch.zeros(NOBS, dtype=torch.int32, device=dev) if want_new_pos else None
    o = _lib.gl_map_add_out()
    o.result, o.already_mp, o.obs_new_pos, o.already_cap = _ptr(result), (_ptr(already) if already_cap else None), _ptr(new_pos), already_cap
    ctx.call(ctx.lib.gl_map_add, NMP, NKF, NFK, NOBS, NMPcap, OBScap, C.byref(ed), _ptr(map.get("mp_pos")), _ptr(ba.get("mp_assoc")), C.byref(ls),
             C.byref(o))
    nmp, nobs, n_att, n_skip, n_already, status = result.tolist()  # the one round trip
    cut = status & (GROW_OBS_TRUNCATED | GROW_MP_TRUNCATED)
    now = (NMP, NKF, NOBS) if cut else (nmp, NKF, nobs)
    m2, b2 = map_views(map, ba, now)
    r = dict(sizes=now, needed=(nmp, NKF, nobs), n_attached=n_att, n_skipped=n_skip, n_already=n_already, status=status,
             already_mp=already[:min(n_already, already_cap)], map=m2, ba=b2)
    if want_new_pos:
        r["obs_new_pos"] = new_pos
    return r


def map_fuse(ctx, map, ba, kf_row, cand_mp, best_idx, sizes=None, repl_cap=None, want_new_pos=False):
    """gl_map_fuse: the matches of ONE key-frame row applied in list order, IN PLACE on the capacity buffers (module docstring).
    cand_mp (n,) i32: the map-point rows given to the search, in its order; best_idx (n,) i32: fuse_search's answer for them (a row of
    it).  Needs ba['kf_uvr'].  -> dict(sizes after the call - those on entry after a truncation, with `needed` - n_fused, n_attached,
    n_replaced, status, repl_src / repl_tgt (min(n_replaced, repl_cap),) i32 in step order, map, ba: cut to sizes[, obs_new_pos (old
    NOBS,) i32: -1 for an entry that is gone]).  After a truncation `needed` holds NOBS + n as its third size: the UPPER BOUND the call
    checks before it runs (every candidate may attach), not the size the edit would produce.  One 20-byte copy and one synchronise."""
    import torch
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, ("kf_uvr",))
    ed = _map_edit(map, ba, None, NMPcap, dev)
    kf_row = int(kf_row)
    assert 0 <= kf_row < NKF, "kf_row %d outside [0, %d)" % (kf_row, NKF)
    n = _tensor("cand_mp", cand_mp, "int32", (None,), dev).shape[0]
    _tensor("best_idx", best_idx, "int32", (n,), dev)
    repl_cap = n if repl_cap is None else int(repl_cap)
    result = torch.zeros(5, dtype=torch.int32, device=dev)
    src = torch.zeros(repl_cap, dtype=torch.int32, device=dev)
    tgt = torch.zeros(repl_cap, dtype=torch.int32, device=dev)
    new_pos = torch.zeros(NOBS, dtype=torch.int32, device=dev) if want_new_pos else None
    o = _lib.gl_map_fuse_out()
    o.result, o.obs_new_pos, o.repl_cap = _ptr(result), _ptr(new_pos), repl_cap
    o.repl_src, o.repl_tgt = (_ptr(src), _ptr(tgt)) if repl_cap else (None, None)
    ctx.call(ctx.lib.gl_map_fuse, NMP, NKF, NFK, NOBS, OBScap, C.byref(ed), _ptr(ba["kf_uvr"]), kf_row, n, _ptr(cand_mp), _ptr(best_idx), C.byref(o))
    nobs, n_fused, n_att, n_repl, status = result.tolist()  # the one round trip
    now = (NMP, NKF, NOBS) if status & GROW_OBS_TRUNCATED else (NMP, NKF, nobs)
    m2, b2 = map_views(map, ba, now)
    k = min(n_repl, repl_cap)
    r = dict(sizes=now, needed=(NMP, NKF, nobs), n_fused=n_fused, n_attached=n_att, n_replaced=n_repl, status=status, repl_src=src[:k], repl_tgt=tgt[:k],
             map=m2, ba=b2)
    if want_new_pos:
        r["obs_new_pos"] = new_pos
    return r


def fuse_observations_from_map(ctx, cam, map, ba, kf_tables, kf_row, cand_mp, th=3.0, scale_factor=1.2, sizes=None, want_new_pos=False):
    """Localization::fuseObservations (localization.cpp:226-321) for ONE key-frame row on the resident map: the candidates' rows gathered
    from the map, project_map_points -> fuse_search -> map_fuse, nothing flattened or uploaded.  map needs the per-point arrays of the
    matchers (mp_pos, mp_normal, mp_max_dist, mp_min_dist, mp_desc), ba kf_pose / kf_twc / kf_uvr / kf_oct; kf_tables: dict(desc
    (key-frame rows, NFK, 32) u8).  cand_mp (n,) i32.  -> the dict of map_fuse + best_idx, best_dist (n,) i32.  A candidate that already
    observes kf_row is matched like any other and dropped by map_fuse's own test (:237)."""
    import torch
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, ("kf_pose", "kf_twc", "kf_uvr", "kf_oct"))
    for k in ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc"):
        assert map.get(k) is not None, "map[%r]: missing" % k
    desc = _tensor("kf_tables['desc']", kf_tables.get("desc"), "uint8", (map["kf_mp"].shape[0], NFK, 32), dev)
    kf_row = int(kf_row)
    assert 0 <= kf_row < NKF, "kf_row %d outside [0, %d)" % (kf_row, NKF)
    n = _tensor("cand_mp", cand_mp, "int32", (None,), dev).shape[0]
    c = cand_mp.long()
    inside = (c >= 0) & (c < NMP)
    c = torch.where(inside, c, torch.zeros_like(c))
    flag = (inside & (map["mp_valid"][c] != 0)).to(torch.uint8)[None].contiguous()
    g = lambda k: map[k][c][None].contiguous()
    uvr, level, _, _, inview = project_map_points(ctx, cam, ba["kf_pose"][kf_row][None].contiguous(), ba["kf_twc"][kf_row][None].contiguous(), g("mp_pos"),
                                                  g("mp_normal"), g("mp_max_dist"), g("mp_min_dist"), flag, scale_factor=scale_factor)
    feat = ba["kf_uvr"][kf_row]
    bi, bd = fuse_search(ctx, cam, feat[None, :, :2].contiguous(), feat[None, :, 2].float().contiguous(), ba["kf_oct"][kf_row][None].contiguous(),
                         desc[kf_row][None].contiguous(), uvr, level, inview, g("mp_desc"), th=th, scale_factor=scale_factor)
    r = map_fuse(ctx, map, ba, kf_row, cand_mp, bi[0], sizes=(NMP, NKF, NOBS), want_new_pos=want_new_pos)
    r.update(best_idx=bi[0], best_dist=bd[0])
    return r


def process_key_frame_from_map(ctx, gmm, cam, prm, map, ba, kf_tables, kf_row, feat_depth, held, th_depth, check_depth=True, k=5, sizes=None,
                               mp_ref_kf=None, scale_factor=1.2):
    """GMMLoc::processKeyFrame's GMM half for ONE key-frame row on the resident map (gmmloc_opt.cpp:20-113): associateMapElements ->
    createMapPointsFromStereo, then the new points' descriptor, normal and distances - GMM.search2d -> api.create_stereo_points ->
    map_add(new_kf = [kf_row], the new rows, their attach triples, the counts on the device) -> api.update_map_points(what = 3) on the
    new rows.  The key-frame's own table rows (ba kf_pose / kf_twc / kf_uvr / kf_oct, kf_tables['desc'] (key-frame rows, NFK, 32) u8) are
    the only upload of the pass; feat_depth (NFK,) f32 and held (NFK,) u8 (api.create_stereo_points) belong to them.  Needs mp_ref_kf
    and the per-point arrays of the matchers in `map`.  One synchronise: map_add's 24-byte read.
    -> the dict of map_add + cand (NFK,k) / ncand (NFK,) i32 (kept for createMapPoints), feat_new (NFK,) i32, stats (8,) i32 (device
    tensors) and n_new.  After a truncation by map_add nothing is changed and nothing refreshed (n_new: what the walk made)."""
    from .api import create_stereo_points, update_map_points
    import torch
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, ("kf_pose", "kf_twc", "kf_uvr", "kf_oct", "mp_assoc"))
    for key in ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc"):
        assert map.get(key) is not None, "map[%r]: missing" % key
    desc = _tensor("kf_tables['desc']", kf_tables.get("desc"), "uint8", (map["kf_mp"].shape[0], NFK, 32), dev)
    rk = _tensor("mp_ref_kf", mp_ref_kf, "int32", (NMPcap,), dev)
    kf_row = int(kf_row)
    assert 0 <= kf_row < NKF, "kf_row %d outside [0, %d)" % (kf_row, NKF)
    _tensor("feat_depth", feat_depth, "float32", (NFK,), dev)
    _tensor("held", held, "uint8", (NFK,), dev)
    uvr = ba["kf_uvr"][kf_row]
    pose, uv = ba["kf_pose"][kf_row][None].contiguous(), uvr[None, :, :2].contiguous()
    cand, ncand, _, _ = gmm.search2d(cam, pose, uv, k=k)
    row = torch.tensor([kf_row], dtype=torch.int32, device=dev)
    s = create_stereo_points(ctx, gmm, cam, prm, dict(pose=pose, feat_uv=uv, feat_ur=uvr[None, :, 2].float().contiguous(), feat_depth=feat_depth[None],
                                                      feat_oct=ba["kf_oct"][kf_row][None].contiguous(), cand=cand, ncand=ncand, held=held[None],
                                                      kf_row=row), NMP, check_depth, th_depth)
    r = map_add(ctx, map, ba, (NMP, NKF, NOBS), new_mp=dict(pos=s["new_pos"][0], assoc=s["new_assoc"][0], ref_kf=s["new_ref_kf"][0]),
                new_kf=row, attach=dict(mp=s["att_mp"][0], kf=s["att_kf"][0], feat=s["att_feat"][0]), mp_ref_kf=rk,
                n_new_mp=s["n_new"], n_attach=s["n_new"])
    n_new = r["needed"][0] - NMP
    if n_new > 0 and not r["status"] & (GROW_OBS_TRUNCATED | GROW_MP_TRUNCATED):
        m2, b2 = r["map"], r["ba"]
        new = slice(NMP, NMP + n_new)
        update_map_points(ctx, dict(twc=b2["kf_twc"], valid=m2["kf_valid"], oct=b2["kf_oct"], desc=desc),
                          dict(pos=m2["mp_pos"][new], valid=m2["mp_valid"][new], ref_kf=rk[new], obs_ptr=m2["obs_ptr"][NMP:], obs_kf=m2["obs_kf"],
                               obs_feat=b2["obs_feat"]),
                          dict(desc=m2["mp_desc"][new], normal=m2["mp_normal"][new], max_dist=m2["mp_max_dist"][new], min_dist=m2["mp_min_dist"][new]),
                          what=3, scale_factor=scale_factor)
    r.update(cand=cand[0], ncand=ncand[0], feat_new=s["feat_new"][0], stats=s["stats"][0], n_new=n_new)
    return r


# ---- createMapPoints on the resident map (gl_tri_pair_setup, gl_create_map_points_from_map; rules in include/gmmloc_hip.h) -----------
TRI_NB_MAX = 16
TRI_SKIP_BEYOND, TRI_SKIP_BAD_ROW, TRI_SKIP_SELF, TRI_SKIP_INVALID, TRI_SKIP_REPEATED, TRI_SKIP_BASELINE = 1, 2, 4, 8, 16, 32
TRI_NONE_SEARCHED = 1
KF_TABLE_DTYPES = {"angle": "float32", "desc": "uint8", "depth": "float32", "nnode": "int32", "node_id": "int32", "node_ptr": "int32",
                   "node_idx": "int32", "cand": "int32", "ncand": "int32"}


def default_mb(cam):
    """Frame::mb = mbf / fx in float (frame.cpp:24)"""
    import numpy as np
    return float(np.float32(cam.bf) / np.float32(cam.fx))


def _kf_tables(kf_tables, rows, NFK, dev):
    """dict of CUDA tensors (keys of KF_TABLE_DTYPES, `rows` key-frame rows each) -> gl_map_kf_tables"""
    for key in kf_tables:
        assert key in KF_TABLE_DTYPES, "kf_tables[%r]: unknown key" % key
    NNcap = _tensor("kf_tables['node_id']", kf_tables.get("node_id"), "int32", (rows, None), dev).shape[1]
    k = _tensor("kf_tables['cand']", kf_tables.get("cand"), "int32", (rows, NFK, None), dev).shape[2]
    shapes = {"angle": (rows, NFK), "desc": (rows, NFK, 32), "depth": (rows, NFK), "nnode": (rows,), "node_id": (rows, NNcap),
              "node_ptr": (rows, NNcap + 1), "node_idx": (rows, NFK), "cand": (rows, NFK, k), "ncand": (rows, NFK)}
    t = _lib.gl_map_kf_tables()
    for key, dt in KF_TABLE_DTYPES.items():
        setattr(t, "kf_" + key, _ptr(_tensor("kf_tables[%r]" % key, kf_tables.get(key), dt, shapes[key], dev)))
    t.NNcap, t.k = NNcap, k
    return t


def _conn(conn_kf, n_conn, dev):
    assert _count("n_conn", n_conn, dev) is not None, "n_conn: missing"
    return _tensor("conn_kf", conn_kf, "int32", (None,), dev).shape[0]


def tri_pair_setup(ctx, cam, ba, kf_valid, kf_row, conn_kf, n_conn, first_nb=0, n_nb=None, mb=None):
    """gl_tri_pair_setup: per neighbour conn_kf[first_nb + j] of key-frame row kf_row the skip bits (TRI_SKIP_*), the fundamental matrix
    and the epipole createMapPoints / searchForTriangulation compute before the search.  ba: kf_pose (NKF,7), kf_twc (NKF,3); kf_valid
    (NKF,) u8 or None; conn_kf (Ccap,) i32 and n_conn (1,) i32 on the device (a row of update_connections' outputs).
    -> (skip (n_nb,) i32, fmat (n_nb,9) f64, epipole (n_nb,2) f32)."""
    import torch
    dev = _tensor("ba['kf_pose']", ba.get("kf_pose"), "float64", (None, 7), None).device
    NKF = ba["kf_pose"].shape[0]
    _tensor("ba['kf_twc']", ba.get("kf_twc"), "float64", (NKF, 3), dev)
    if kf_valid is not None:
        _tensor("kf_valid", kf_valid, "uint8", (NKF,), dev)
    cap = _conn(conn_kf, n_conn, dev)
    n_nb = min(cap, TRI_NB_MAX) if n_nb is None else int(n_nb)
    skip = torch.zeros(n_nb, dtype=torch.int32, device=dev)
    fmat = torch.zeros((n_nb, 9), dtype=torch.float64, device=dev)
    epi = torch.zeros((n_nb, 2), dtype=torch.float32, device=dev)
    ctx.call(ctx.lib.gl_tri_pair_setup, C.byref(cam.c()), NKF, _ptr(kf_valid), _ptr(ba["kf_pose"]), _ptr(ba["kf_twc"]), int(kf_row), _ptr(conn_kf),
             _ptr(n_conn), cap, int(first_nb), n_nb, default_mb(cam) if mb is None else float(mb), _ptr(skip), _ptr(fmat), _ptr(epi))
    return skip, fmat, epi


def tri_points_out(NFK, n_nb, new_cap=None, device="cuda"):
    """the output arrays of create_map_points_on_map, zeroed: the lists of new_cap (default NFK) rows, att_* twice as many"""
    import torch
    cap = NFK if new_cap is None else int(new_cap)
    z = lambda *sh: torch.zeros(sh, dtype=torch.int32, device=device)
    return dict(new_pos=torch.zeros((cap, 3), dtype=torch.float64, device=device), new_assoc=z(cap), new_ref_kf=z(cap), new_type=z(cap), new_nb=z(cap),
                new_feat1=z(cap), new_feat2=z(cap), att_mp=z(2 * cap), att_kf=z(2 * cap), att_feat=z(2 * cap), n_new=z(1), n_attach=z(1),
                feat_new=z(NFK), nb_stats=z(n_nb, 8), fmat=torch.zeros((n_nb, 9), dtype=torch.float64, device=device),
                epipole=torch.zeros((n_nb, 2), dtype=torch.float32, device=device), status=z(1))


def create_map_points_on_map(ctx, gmm, cam, prm, map, ba, kf_tables, kf_row, conn_kf, n_conn, first_nb=0, n_nb=None, mb=None, mp_base=None,
                             scale_factor=1.2, out=None):
    """gl_create_map_points_from_map alone: the loop of Localization::createMapPoints for key-frame row kf_row over the neighbours
    conn_kf[first_nb .. first_nb + n_nb) - the map is NOT written, nothing is read back.  map / ba: the dicts of api.update_connections /
    api.ba_window_build cut to the map's sizes (kf_valid, kf_mp; kf_pose, kf_twc, kf_uvr, kf_oct); kf_tables: dict of KF_TABLE_DTYPES'
    keys, one row per key-frame row of map['kf_mp'].  mp_base: the row the first new point will take (default: the map's NMP).
    -> the dict of tri_points_out (device tensors; the lists are valid up to n_new / n_attach)."""
    v, dev = _map_view(map, False)
    w = _map_ba_view(ba, v, dev, need=("kf_pose", "kf_twc", "kf_uvr", "kf_oct"))
    assert ba.get("kf_twc") is not None, "ba['kf_twc']: missing"
    t = _kf_tables(kf_tables, v.NKF, v.NFK, dev)
    cap = _conn(conn_kf, n_conn, dev)
    n_nb = min(cap, TRI_NB_MAX) if n_nb is None else int(n_nb)
    if out is None:
        out = tri_points_out(v.NFK, n_nb, device=dev)
    o = _lib.gl_tri_points_out()
    shapes = {"new_pos": (None, 3), "fmat": (n_nb, 9), "epipole": (n_nb, 2), "nb_stats": (n_nb, 8), "feat_new": (v.NFK,), "n_new": (1,),
              "n_attach": (1,), "status": (1,)}
    for key in _lib.TRI_POINTS_ARRAYS:
        dt = "float64" if key in ("new_pos", "fmat") else "float32" if key == "epipole" else "int32"
        if out.get(key) is None and key in ("fmat", "epipole"):
            continue
        setattr(o, key, _ptr(_tensor("out[%r]" % key, out.get(key), dt, shapes.get(key, (None,)), dev)))
    o.new_cap = out["new_pos"].shape[0]
    for key in ("new_assoc", "new_ref_kf", "new_type", "new_nb", "new_feat1", "new_feat2"):
        assert out[key].shape[0] == o.new_cap, "out[%r]: %d rows, new_pos has %d" % (key, out[key].shape[0], o.new_cap)
    for key in ("att_mp", "att_kf", "att_feat"):
        assert out[key].shape[0] == 2 * o.new_cap, "out[%r]: needs 2 x %d entries" % (key, o.new_cap)
    ctx.call(ctx.lib.gl_create_map_points_from_map, gmm.h, C.byref(cam.c()), C.byref(prm.c()), float(scale_factor), C.byref(v), C.byref(w),
             C.byref(t), int(kf_row), _ptr(conn_kf), _ptr(n_conn), cap, int(first_nb), n_nb, default_mb(cam) if mb is None else float(mb),
             v.NMP if mp_base is None else int(mp_base), C.byref(o))
    return out


def create_map_points_from_map(ctx, gmm, cam, prm, map, ba, kf_tables, kf_row, nn=10, mb=None, first_nb=0, sizes=None, mp_ref_kf=None,
                               scale_factor=1.2):
    """Localization::createMapPoints (localization_opt.cpp:206-454) for ONE key-frame row on the resident map: api.update_connections
    (kf_row) -> create_map_points_on_map over its neighbours [first_nb, first_nb + nn) -> map_add(the new rows, their attach triples, the
    counts on the device) -> api.update_map_points(what = 3) on the new rows.  map / ba: the capacity buffers of this module with `sizes`;
    needs the per-point arrays of the matchers, ba kf_pose / kf_twc / kf_uvr / kf_oct / mp_assoc and mp_ref_kf; kf_tables: dict of
    KF_TABLE_DTYPES' keys over the key-frame rows of the buffers.  mb defaults to float32(cam.bf) / float32(cam.fx) (frame.cpp:24).
    One synchronise: map_add's 24-byte read.
    -> the dict of map_add + new_type, new_nb, feat_new, nb_stats (device tensors; new_type / new_nb cut to n_new) and n_new.  The host's
    candidate_mappts_ gains the rows [NMP, NMP + n_new) and type_ comes from new_type.  After a truncation by map_add nothing is changed
    and nothing refreshed (n_new: what the loop made)."""
    from .api import update_connections, update_map_points
    import torch
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, ("kf_pose", "kf_twc", "kf_uvr", "kf_oct", "mp_assoc"))
    for key in ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc"):
        assert map.get(key) is not None, "map[%r]: missing" % key
    rk = _tensor("mp_ref_kf", mp_ref_kf, "int32", (NMPcap,), dev)
    kf_row, nn = int(kf_row), int(nn)
    assert 0 <= kf_row < NKF, "kf_row %d outside [0, %d)" % (kf_row, NKF)
    m1, b1 = map_views(map, ba, (NMP, NKF, NOBS))
    kt = {key: t[:NKF] for key, t in kf_tables.items()}
    view = {key: m1[key] for key in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")}
    conn = update_connections(ctx, view, torch.tensor([kf_row], dtype=torch.int32, device=dev), Ccap=max(first_nb + nn, 1))
    s = create_map_points_on_map(ctx, gmm, cam, prm, view, {key: b1[key] for key in ("kf_pose", "kf_twc", "kf_uvr", "kf_oct")}, kt, kf_row,
                                 conn["conn_kf"][0], conn["n_conn"], first_nb=first_nb, n_nb=nn, mb=mb, mp_base=NMP, scale_factor=scale_factor)
    r = map_add(ctx, map, ba, (NMP, NKF, NOBS), new_mp=dict(pos=s["new_pos"], assoc=s["new_assoc"], ref_kf=s["new_ref_kf"]),
                attach=dict(mp=s["att_mp"], kf=s["att_kf"], feat=s["att_feat"]), mp_ref_kf=rk, n_new_mp=s["n_new"], n_attach=s["n_attach"])
    n_new = r["needed"][0] - NMP
    if n_new > 0 and not r["status"] & (GROW_OBS_TRUNCATED | GROW_MP_TRUNCATED):
        m2, b2 = r["map"], r["ba"]
        new = slice(NMP, NMP + n_new)
        update_map_points(ctx, dict(twc=b2["kf_twc"], valid=m2["kf_valid"], oct=b2["kf_oct"], desc=kt["desc"]),
                          dict(pos=m2["mp_pos"][new], valid=m2["mp_valid"][new], ref_kf=rk[new], obs_ptr=m2["obs_ptr"][NMP:], obs_kf=m2["obs_kf"],
                               obs_feat=b2["obs_feat"]),
                          dict(desc=m2["mp_desc"][new], normal=m2["mp_normal"][new], max_dist=m2["mp_max_dist"][new], min_dist=m2["mp_min_dist"][new]),
                          what=3, scale_factor=scale_factor)
    r.update(new_type=s["new_type"][:n_new], new_nb=s["new_nb"][:n_new], feat_new=s["feat_new"], nb_stats=s["nb_stats"], n_new=n_new)
    return r
