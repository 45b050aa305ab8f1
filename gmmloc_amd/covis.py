"""The covisibility graph as part of the resident map and Localization::searchInNeighbors on it: gl_covis_update, gl_covis_remove,
gl_covis_best, gl_fuse_targets, gl_fuse_candidates; rules, reproduced quirks and declared deviations in include/gmmloc_hip.h
(gl_map_covis).

`cov` is the dict of covis_alloc: cov_kf / cov_w (NKFcap, Wcap) i32, cov_n / cov_nord / best_cov (NKFcap,) i32.  A row holds
map_frame_weights_ in the declared order (weight descending, ties to the lowest row); ordered_keyframes_ is its first cov_nord entries.
Every wrapper only enqueues and returns device tensors; update_connections_in_map and search_in_neighbors_from_map say what they read."""
import ctypes as C

from . import _lib, map_grow
from ._host import _count, _map_buffers, _map_view, _ptr, _tensor

CONN_KEPT, CONN_TRUNCATED, CONN_BAD_ROW = 1, 2, 4
COVIS_W_TRUNCATED, COVIS_EMPTY_LIST, COVIS_BAD_ROW, COVIS_LIST_TRUNCATED = 8, 16, 32, 64
_KEYS = ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov")


def covis_alloc(NKFcap, Wcap, device="cuda"):
    """the graph of a map without connections: every row empty, best_cov = -1"""
    import torch
    z = lambda *sh: torch.zeros(sh, dtype=torch.int32, device=device)
    return dict(cov_kf=z(int(NKFcap), int(Wcap)), cov_w=z(int(NKFcap), int(Wcap)), cov_n=z(int(NKFcap)), cov_nord=z(int(NKFcap)),
                best_cov=torch.full((int(NKFcap),), -1, dtype=torch.int32, device=device))


def grow_tables(cov, Wcap):
    """the same graph with rows of Wcap >= the present width entries (what a call that set COVIS_W_TRUNCATED asks for in result[0]):
    cov_kf / cov_w re-strided, the other arrays shared"""
    import torch
    old = cov["cov_kf"].shape[1]
    Wcap = int(Wcap)
    assert Wcap >= old, "Wcap %d below the present %d" % (Wcap, old)
    out = dict(cov)
    for k in ("cov_kf", "cov_w"):
        t = torch.zeros((cov[k].shape[0], Wcap), dtype=torch.int32, device=cov[k].device)
        t[:, :old] = cov[k]
        out[k] = t
    return out


def _cov(cov, dev=None):
    """dict -> (gl_map_covis, NKFcap, Wcap, device)"""
    for k in cov:
        assert k in _KEYS, "cov[%r]: unknown key" % k
    t = _tensor("cov['cov_kf']", cov.get("cov_kf"), "int32", (None, None), dev)
    dev = t.device
    NKFcap, Wcap = t.shape
    assert Wcap >= 1, "cov['cov_kf']: rows of at least one entry"
    _tensor("cov['cov_w']", cov.get("cov_w"), "int32", (NKFcap, Wcap), dev)
    s = _lib.gl_map_covis()
    s.NKFcap, s.Wcap = NKFcap, Wcap
    s.cov_kf, s.cov_w = _ptr(cov["cov_kf"]), _ptr(cov["cov_w"])
    for k in ("cov_n", "cov_nord", "best_cov"):
        setattr(s, k, _ptr(_tensor("cov[%r]" % k, cov.get(k), "int32", (NKFcap,), dev)))
    return s, NKFcap, Wcap, dev


def _zeros(n, dev):
    import torch
    return torch.zeros(n, dtype=torch.int32, device=dev)


def covis_update(ctx, map, cov, kf_row, Ccap=256):
    """gl_covis_update: KeyFrame::updateConnections with its addConnection on the other rows, for key-frame row kf_row of `map` (the dict
    of api.update_connections, cut to the map's sizes); `cov` IN PLACE.  -> dict(conn_kf, conn_w (Ccap,) i32, n_conn (1,) i32: as
    api.update_connections' row; result (4,) i32 = {widest row, status, other rows changed, 0}).  After COVIS_W_TRUNCATED the graph is
    untouched and result[0] is the Wcap the call needs (grow_tables)."""
    v, dev = _map_view(map, False)
    s, NKFcap, _, _ = _cov(cov, dev)
    assert v.NKF <= NKFcap, "the map has %d key-frame rows, the graph %d" % (v.NKF, NKFcap)
    kf_row, Ccap = int(kf_row), int(Ccap)
    assert 0 <= kf_row < v.NKF, "kf_row %d outside [0, %d)" % (kf_row, v.NKF)
    out = dict(conn_kf=_zeros(Ccap, dev), conn_w=_zeros(Ccap, dev), n_conn=_zeros(1, dev), result=_zeros(4, dev))
    ctx.call(ctx.lib.gl_covis_update, C.byref(v), C.byref(s), kf_row, Ccap, _ptr(out["conn_kf"]), _ptr(out["conn_w"]), _ptr(out["n_conn"]),
             _ptr(out["result"]))
    return out


def update_connections_in_map(ctx, map, cov, kf_row, Ccap=256):
    """covis_update, and after COVIS_W_TRUNCATED grow_tables to the width it asked for and the call again.  -> (the dict of
    covis_update, cov - the same dict, or the re-strided one).  One 16-byte read of result per attempt."""
    out = covis_update(ctx, map, cov, kf_row, Ccap)
    res = out["result"].tolist()
    if res[1] & COVIS_W_TRUNCATED:
        cov = grow_tables(cov, res[0])
        out = covis_update(ctx, map, cov, kf_row, Ccap)
    return out, cov


def covis_remove(ctx, cov, NKF, cull_rows, n_cull=None, kf_first=-1):
    """gl_covis_remove: the graph part of Map::removeKeyFrame for cull_rows (cap,) i32 IN REMOVAL ORDER (cull_rows / n_cull of
    api.cull_keyframes; n_cull (1,) i32 on the device clamps the length); `cov` IN PLACE, beside api.map_remove(rm_kf).
    -> result (4,) i32 = {rows removed, status, entries erased, rows skipped as malformed}."""
    s, NKFcap, _, dev = _cov(cov)
    NKF = int(NKF)
    assert 0 <= NKF <= NKFcap, "NKF %d outside [0, %d]" % (NKF, NKFcap)
    cap = _tensor("cull_rows", cull_rows, "int32", (None,), dev).shape[0]
    result = _zeros(4, dev)
    ctx.call(ctx.lib.gl_covis_remove, NKF, C.byref(s), int(kf_first), _ptr(cull_rows) if cap else None, _count("n_cull", n_cull, dev), cap, _ptr(result))
    return result


def covis_best(ctx, cov, NKF, kf_row, N=0, Ccap=256):
    """gl_covis_best: getBestCovisibilityKeyFrames(N) (N <= 0: getVectorCovisibleKeyFrames) of the rows kf_row (B,) i32.
    -> dict(conn_kf, conn_w (B,Ccap) i32, n_conn (B,) i32: the shape of api.update_connections' outputs; result (4,) i32)."""
    s, NKFcap, _, dev = _cov(cov)
    NKF, Ccap = int(NKF), int(Ccap)
    assert 0 <= NKF <= NKFcap, "NKF %d outside [0, %d]" % (NKF, NKFcap)
    B = _tensor("kf_row", kf_row, "int32", (None,), dev).shape[0]
    import torch
    out = dict(conn_kf=torch.zeros((B, Ccap), dtype=torch.int32, device=dev), conn_w=torch.zeros((B, Ccap), dtype=torch.int32, device=dev),
               n_conn=_zeros(B, dev), result=_zeros(4, dev))
    ctx.call(ctx.lib.gl_covis_best, NKF, C.byref(s), B, _ptr(kf_row), int(N), Ccap, _ptr(out["conn_kf"]), _ptr(out["conn_w"]), _ptr(out["n_conn"]),
             _ptr(out["result"]))
    return out


def fuse_targets(ctx, cov, kf_valid, NKF, kf_row, nn=10, nn2=5, Tcap=None):
    """gl_fuse_targets: the target key-frames of searchInNeighbors for key-frame row kf_row, in INSERTION order.  kf_valid (>= NKF,) u8
    or None.  -> dict(tgt_kf (Tcap,) i32, n_tgt (1,) i32 - views of ONE tensor `list` = [n_tgt | tgt_kf], so that one copy reads both -,
    result (4,) i32 = {count, status, 0, malformed entries}).  Tcap defaults to nn + nn * nn2, which always suffices."""
    s, NKFcap, _, dev = _cov(cov)
    NKF, nn, nn2 = int(NKF), int(nn), int(nn2)
    assert 0 <= NKF <= NKFcap, "NKF %d outside [0, %d]" % (NKF, NKFcap)
    assert 0 <= int(kf_row) < NKF, "kf_row %d outside [0, %d)" % (int(kf_row), NKF)
    if kf_valid is not None:
        assert _tensor("kf_valid", kf_valid, "uint8", (None,), dev).shape[0] >= NKF, "kf_valid: fewer than NKF rows"
    Tcap = nn + nn * nn2 if Tcap is None else int(Tcap)
    buf = _zeros(1 + Tcap, dev)
    out = dict(list=buf, n_tgt=buf[:1], tgt_kf=buf[1:], result=_zeros(4, dev))
    ctx.call(ctx.lib.gl_fuse_targets, NKF, C.byref(s), _ptr(kf_valid), int(kf_row), nn, nn2, Tcap, _ptr(out["tgt_kf"]) if Tcap else None,
             _ptr(out["n_tgt"]), _ptr(out["result"]))
    return out


def fuse_candidates(ctx, map, tgt_kf, n_tgt, kf_idx, cand_cap=None):
    """gl_fuse_candidates: the candidates of the reverse fuse - the valid points of the targets tgt_kf (Tcap,) i32 / n_tgt (1,) i32 (of
    fuse_targets), each at its first occurrence, on `map` (mp_valid, kf_mp, ...) AS IT IS NOW.  kf_idx = curr_kf_->idx_ (0: the list is
    empty, as in the reference).  cand_cap defaults to Tcap x NFK, which always suffices.
    -> dict(cand_mp (cand_cap,) i32, n_cand (1,) i32, result (4,) i32 = {count, status, 0, targets outside the table})."""
    v, dev = _map_view(map, False)
    Tcap = _tensor("tgt_kf", tgt_kf, "int32", (None,), dev).shape[0]
    assert _count("n_tgt", n_tgt, dev) is not None, "n_tgt: missing"
    cand_cap = Tcap * v.NFK if cand_cap is None else int(cand_cap)
    out = dict(cand_mp=_zeros(cand_cap, dev), n_cand=_zeros(1, dev), result=_zeros(4, dev))
    ctx.call(ctx.lib.gl_fuse_candidates, C.byref(v), _ptr(tgt_kf) if Tcap else None, _ptr(n_tgt), Tcap, int(kf_idx), cand_cap,
             _ptr(out["cand_mp"]) if cand_cap else None, _ptr(out["n_cand"]), _ptr(out["result"]))
    return out


def _view(m):
    return {k: m[k] for k in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")}


def refresh_points(ctx, map, ba, kf_tables, mp_ref_kf, sizes, rows, what, scale_factor=1.2):
    """gl_update_map_points(what) on the VALID points among the map-point rows `rows` (any i32 device tensor; entries outside [0, NMP)
    are ignored), in place in the map's arrays: the whole map goes to the call with a mask as its pt_valid, so nothing is gathered and
    nothing read back."""
    import torch
    from .api import update_map_points
    NMP, NKF, _ = sizes
    m, b = map_grow.map_views(map, ba, sizes)
    r = rows.reshape(-1).long()
    mask = torch.zeros(NMP + 1, dtype=torch.uint8, device=r.device)
    mask[torch.where((r >= 0) & (r < NMP), r, torch.full_like(r, NMP))] = 1
    mask = (mask[:NMP] & (m["mp_valid"] != 0).to(torch.uint8)).contiguous()
    update_map_points(ctx, dict(twc=b["kf_twc"], valid=m["kf_valid"], oct=b["kf_oct"], desc=kf_tables["desc"][:NKF]),
                      dict(pos=m["mp_pos"], valid=mask, ref_kf=None if mp_ref_kf is None else mp_ref_kf[:NMP], obs_ptr=m["obs_ptr"], obs_kf=m["obs_kf"],
                           obs_feat=b["obs_feat"]),
                      dict(desc=m["mp_desc"], normal=m["mp_normal"], max_dist=m["mp_max_dist"], min_dist=m["mp_min_dist"]), what=what,
                      scale_factor=scale_factor)


def fuse_and_note(ctx, cam, map, ba, kf_tables, kf, cand_mp, sizes, stats=None, mp_replaced=None, th=3.0, scale_factor=1.2):
    """one fuseObservations of searchInNeighbors with what Map::replaceMapPoint does beside the observations: map_grow.
    fuse_observations_from_map, then the descriptor of the repl_tgt rows (map.cpp:144), gl_map_stats_merge and gl_map_note_replaced on
    repl_src / repl_tgt.  -> the dict of fuse_observations_from_map"""
    from . import frame_step, map_stats
    r = map_grow.fuse_observations_from_map(ctx, cam, map, ba, kf_tables, kf, cand_mp, th=th, scale_factor=scale_factor, sizes=sizes)
    if r["repl_src"].shape[0] > 0:
        refresh_points(ctx, map, ba, kf_tables, None, r["sizes"], r["repl_tgt"], 1, scale_factor)
        if stats is not None:
            map_stats.map_stats_merge(ctx, stats, r["sizes"][0], r["repl_src"], r["repl_tgt"])
        if mp_replaced is not None:
            frame_step.note_replaced(ctx, mp_replaced, r["repl_src"], r["repl_tgt"])
    return r


def search_in_neighbors_from_map(ctx, cam, map, ba, cov, kf_tables, kf_row, kf_idx, stats=None, mp_replaced=None, mp_ref_kf=None, sizes=None,
                                 th=3.0, scale_factor=1.2, nn=10, nn2=5, Ccap=256):
    """Localization::searchInNeighbors (localization.cpp:154-224) for key-frame row kf_row (idx_ = kf_idx) on the resident map and its
    graph.  map / ba: the capacity buffers of map_grow with `sizes`; needs the per-point arrays of the matchers, ba kf_pose / kf_twc /
    kf_uvr / kf_oct, kf_tables['desc'] and mp_ref_kf (NMPcap,) i32 (updateNormalAndDepth reads ref_kf_); stats: the dict of map_stats,
    mp_replaced (NMPcap,) i32 - both optional.  In order:
      1  fuse_targets, and ONE read of n_tgt with the list (4 + 4 (nn + nn nn2) bytes in one copy: gl_map_fuse takes its row from the host)
      2  a COPY of kf_mp[kf_row]: curr_mappts is a snapshot (:182) - a point replaced at an earlier target stays in it, invalid
      3  per target, in order: fuse_and_note with the snapshot as candidates
      4  fuse_candidates on the map as it is then, ONE 4-byte read of n_cand (gl_map_fuse refuses a list that OBScap could not take if
         every entry attached, so the list cannot go padded) -> fuse_and_note into kf_row itself
      5  gl_update_map_points(what = 3) on the valid points kf_row holds now (:213-219)
      6  gl_covis_update(kf_row) (:223)
    Reads per call: the one of step 1, the one of step 4, and gl_map_fuse's 20 bytes per fuse (n_tgt + 1 of them), as map_grow.map_fuse has them today.
    A fuse that OBScap refuses (GROW_OBS_TRUNCATED) ends the loop: `status` carries the bit and the steps after it are not run.
    -> dict(sizes, map, ba: after the call; tgt_kf: the list (host); n_fused, n_attached, n_replaced: per fuse, the reverse one last;
    n_cand (host); conn: the dict of covis_update or None; status: the bits of the calls or-ed - the fuses', COVIS_*)."""
    NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev = _map_buffers(map, ba, sizes, ("kf_pose", "kf_twc", "kf_uvr", "kf_oct"))
    rk = _tensor("mp_ref_kf", mp_ref_kf, "int32", (NMPcap,), dev)
    kf_row = int(kf_row)
    assert 0 <= kf_row < NKF, "kf_row %d outside [0, %d)" % (kf_row, NKF)
    tg = fuse_targets(ctx, cov, map["kf_valid"], NKF, kf_row, nn, nn2)
    head = tg["list"].tolist()  # the one read
    targets = head[1:1 + head[0]]
    status = 0
    snapshot = map["kf_mp"][kf_row].clone()
    cur = (NMP, NKF, NOBS)
    counts = dict(n_fused=[], n_attached=[], n_replaced=[])
    def fuse(kf, cand):
        nonlocal cur, status
        r = fuse_and_note(ctx, cam, map, ba, kf_tables, kf, cand, cur, stats, mp_replaced, th, scale_factor)
        cur, status = r["sizes"], status | r["status"]
        for k in counts:
            counts[k].append(r[k])
        return not r["status"] & map_grow.GROW_OBS_TRUNCATED
    ok = all(fuse(k, snapshot) for k in targets)
    n_cand, conn = None, None
    if ok:
        m1, _ = map_grow.map_views(map, ba, cur)
        cd = fuse_candidates(ctx, _view(m1), tg["tgt_kf"], tg["n_tgt"], kf_idx)
        n_cand = int(cd["n_cand"].item())  # the second read
        ok = fuse(kf_row, cd["cand_mp"][:n_cand].contiguous())
    if ok:
        refresh_points(ctx, map, ba, kf_tables, rk, cur, map["kf_mp"][kf_row], 3, scale_factor)
        m1, _ = map_grow.map_views(map, ba, cur)
        conn = covis_update(ctx, _view(m1), cov, kf_row, Ccap)
    m2, b2 = map_grow.map_views(map, ba, cur)
    return dict(sizes=cur, map=m2, ba=b2, tgt_kf=targets, n_cand=n_cand, conn=conn, status=status, **counts)
