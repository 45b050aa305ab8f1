"""The resident map's found / visible counters and Localization::removeMapPoints on the device: gl_map_stats_track,
gl_map_stats_new_points, gl_map_cand_append, gl_map_stats_merge, gl_cull_map_points; rules in include/gmmloc_hip.h.

`stats` is the dict of map_stats_alloc: visible / found / ref_idx (NMPcap,) i32 beside the per-point capacity buffers of map_grow, cand
(cand_cap,) i32 with n_cand (1,) i32 = candidate_mappts_ as map-point rows, and kf_idx (key-frame rows,) i32 or None (idx_ = the row).
Every wrapper only enqueues: what it returns are device tensors, nothing is read back."""
import ctypes as C

from . import _lib
from ._host import _count, _map_ba_view, _map_edit, _map_view, _outputs, _ptr, _tensor

STATS_MP_TRUNCATED, STATS_CAND_TRUNCATED, STATS_BAD_ROW = 1, 2, 4
VERDICT_KEPT, VERDICT_INVALID, VERDICT_RATIO, VERDICT_YOUNG_FEW, VERDICT_AGED, VERDICT_BAD_ROW = 0, 1, 2, 3, 4, 5


def map_stats_alloc(NMPcap, cand_cap, kf_idx=None, device="cuda"):
    """the counters of an empty map: visible = found = 0, ref_idx = -1 (mappoint.h:86), an empty candidate list"""
    import torch
    z = lambda n: torch.zeros(int(n), dtype=torch.int32, device=device)
    return dict(visible=z(NMPcap), found=z(NMPcap), ref_idx=torch.full((int(NMPcap),), -1, dtype=torch.int32, device=device), kf_idx=kf_idx,
                cand=z(cand_cap), n_cand=z(1))


def _stats(stats, dev=None):
    """dict -> (gl_map_stats, NMPcap, device)"""
    for k in stats:
        assert k in ("visible", "found", "ref_idx", "kf_idx", "cand", "n_cand"), "stats[%r]: unknown key" % k
    v = _tensor("stats['visible']", stats.get("visible"), "int32", (None,), dev)
    dev, NMPcap = v.device, v.shape[0]
    s = _lib.gl_map_stats()
    s.mp_visible = _ptr(v)
    s.mp_found = _ptr(_tensor("stats['found']", stats.get("found"), "int32", (NMPcap,), dev))
    s.mp_ref_idx = _ptr(_tensor("stats['ref_idx']", stats.get("ref_idx"), "int32", (NMPcap,), dev))
    if stats.get("kf_idx") is not None:
        s.kf_idx = _ptr(_tensor("stats['kf_idx']", stats["kf_idx"], "int32", (None,), dev))
    s.cand_cap = _tensor("stats['cand']", stats.get("cand"), "int32", (None,), dev).shape[0]
    s.cand = _ptr(stats["cand"]) if s.cand_cap else None
    s.n_cand = _ptr(_tensor("stats['n_cand']", stats.get("n_cand"), "int32", (1,), dev))
    return s, NMPcap, dev


def map_stats_track(ctx, stats, NMP, feat_mp, match_local, outlier, inview, local_mp, n_local_mp, counts2=None):
    """gl_map_stats_track: the tracker's three rules for B frames on the chain's outputs - feat_mp / match_local (B,NF) i32, outlier
    (B,NF) u8, inview (B,NPcap) u8, local_mp (B,NPcap) i32, n_local_mp (B,) i32, counts2 (B,4) i32 or None (every frame tracked).
    stats['visible'] / ['found'] IN PLACE, rows [0, NMP)."""
    s, NMPcap, dev = _stats(stats)
    NMP = int(NMP)
    assert 0 <= NMP <= NMPcap, "NMP %d outside [0, %d]" % (NMP, NMPcap)
    B, NF = _tensor("feat_mp", feat_mp, "int32", (None, None), dev).shape
    _tensor("match_local", match_local, "int32", (B, NF), dev)
    _tensor("outlier", outlier, "uint8", (B, NF), dev)
    NPcap = _tensor("local_mp", local_mp, "int32", (B, None), dev).shape[1]
    _tensor("inview", inview, "uint8", (B, NPcap), dev)
    _tensor("n_local_mp", n_local_mp, "int32", (B,), dev)
    if counts2 is not None:
        _tensor("counts2", counts2, "int32", (B, 4), dev)
    ctx.call(ctx.lib.gl_map_stats_track, NMP, C.byref(s), B, NF, NPcap, _ptr(feat_mp), _ptr(match_local), _ptr(outlier), _ptr(inview),
             _ptr(local_mp), _ptr(n_local_mp), _ptr(counts2))


def map_stats_new_points(ctx, stats, NKF, first, new_ref_kf, n=None, n_dev=None):
    """gl_map_stats_new_points: rows [first, first + n) get visible = found = 1 and ref_idx from new_ref_kf (n,) i32 (the list map_add
    took); n defaults to the tensor's length, n_dev (1,) i32 on the device clamps it (n_new_mp of map_add).  -> status (1,) i32."""
    import torch
    s, NMPcap, dev = _stats(stats)
    cap = _tensor("new_ref_kf", new_ref_kf, "int32", (None,), dev).shape[0]
    n = cap if n is None else int(n)
    assert 0 <= n <= cap, "n %d outside [0, %d]" % (n, cap)
    if stats.get("kf_idx") is not None:
        assert stats["kf_idx"].shape[0] >= int(NKF), "stats['kf_idx']: fewer than NKF rows"
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.call(ctx.lib.gl_map_stats_new_points, NMPcap, int(NKF), C.byref(s), int(first), n, _count("n_dev", n_dev, dev), _ptr(new_ref_kf), _ptr(status))
    return status


def map_cand_append(ctx, stats, rows=None, n_dev=None, first=0, n=None):
    """gl_map_cand_append: `rows` (cap,) i32 (already_mp of map_add; n defaults to its length) or, with rows None, the range
    [first, first + n) is appended to stats['cand'] at stats['n_cand']; n_dev (1,) i32 clamps n.  -> result (2,) i32 = {the list's size
    afterwards - the size NEEDED after STATS_CAND_TRUNCATED, when nothing was appended -, status}."""
    import torch
    s, _, dev = _stats(stats)
    if rows is not None:
        cap = _tensor("rows", rows, "int32", (None,), dev).shape[0]
        n = cap if n is None else int(n)
        assert 0 <= n <= cap, "n %d outside [0, %d]" % (n, cap)
    else:
        assert n is not None, "a row range needs n"
    result = torch.zeros(2, dtype=torch.int32, device=dev)
    ctx.call(ctx.lib.gl_map_cand_append, C.byref(s), _ptr(rows), int(first), int(n), _count("n_dev", n_dev, dev), _ptr(result))
    return result


def map_stats_merge(ctx, stats, NMP, repl_src, repl_tgt, n=None, n_dev=None):
    """gl_map_stats_merge: repl_src / repl_tgt of map_fuse in step order, tgt += src on both counters IN PLACE; n defaults to the
    tensors' length, n_dev (1,) i32 clamps it (result[3] of gl_map_fuse)."""
    s, NMPcap, dev = _stats(stats)
    NMP = int(NMP)
    assert 0 <= NMP <= NMPcap, "NMP %d outside [0, %d]" % (NMP, NMPcap)
    cap = _tensor("repl_src", repl_src, "int32", (None,), dev).shape[0]
    _tensor("repl_tgt", repl_tgt, "int32", (cap,), dev)
    n = cap if n is None else int(n)
    assert 0 <= n <= cap, "n %d outside [0, %d]" % (n, cap)
    ctx.call(ctx.lib.gl_map_stats_merge, NMP, C.byref(s), _ptr(repl_src), _ptr(repl_tgt), n, _count("n_dev", n_dev, dev))


def cull_map_points(ctx, map, ba, stats, kf_row, out=None):
    """gl_cull_map_points: Localization::removeMapPoints for key-frame row kf_row on the UNEDITED map.  map / ba: the dicts of
    api.map_remove cut to the map's sizes (mp_valid, kf_mp, obs_ptr, obs_kf; kf_uvr, obs_feat).  stats['cand'] / ['n_cand'] are compacted
    IN PLACE.  -> dict(rm_mp (cand_cap,) i32, n_rm (1,) i32: rm_mp / n_rm_mp of api.map_remove; verdict (cand_cap,) i32: the old entries;
    result (4,) i32 = {kept, removed, erased without removal, status}), device tensors.  out: the dict of an earlier call, used again."""
    v, dev = _map_view(map, False)
    _map_ba_view(ba, v, dev, need=("kf_uvr", "obs_feat"))
    assert map.get("mp_valid") is not None, "map['mp_valid']: missing"
    s, NMPcap, _ = _stats(stats, dev)
    assert v.NMP <= NMPcap, "the map has %d points, the counters %d rows" % (v.NMP, NMPcap)
    if stats.get("kf_idx") is not None:
        assert stats["kf_idx"].shape[0] >= v.NKF, "stats['kf_idx']: fewer than NKF rows"
    kf_row = int(kf_row)
    assert 0 <= kf_row < v.NKF, "kf_row %d outside [0, %d)" % (kf_row, v.NKF)
    ed = _map_edit(map, ba, None, v.NMP, dev)  # (kf_valid may be missing: all valid)
    cap = s.cand_cap
    out = _outputs(out, {k: ("int32", (n,), 0) for k, n in (("rm_mp", cap), ("n_rm", 1), ("verdict", cap), ("result", 4))}, dev)
    ctx.call(ctx.lib.gl_cull_map_points, v.NMP, v.NKF, v.NFK, v.NOBS, C.byref(ed), _ptr(ba["kf_uvr"]), C.byref(s), kf_row,
             _ptr(out["rm_mp"]) if cap else None, _ptr(out["n_rm"]), _ptr(out["verdict"]) if cap else None, _ptr(out["result"]))
    return out


def track_frame_with_stats(ctx, cam, prm, a, map, lm, stats, **kw):
    """api.track_frame_chain_map, then gl_map_stats_track on the tensors it returned and the local map it left in `lm`: the tracked
    frame with its num_visible_ / num_found_ bookkeeping, no copy to the host.  -> the dict of track_frame_chain_map."""
    from .api import track_frame_chain_map
    out = track_frame_chain_map(ctx, cam, prm, a, map, lm, **kw)
    map_stats_track(ctx, stats, map["obs_ptr"].shape[0] - 1, out["feat_mp"], out["match_local"], out["outlier"], out["inview"], lm["local_mp"],
                    lm["n_local_mp"], out["counts2"])
    return out


def remove_map_points_from_map(ctx, map, ba, stats, kf_row, mp_ref_kf=None, want_new_pos=False):
    """Localization::removeMapPoints (localization.cpp:127-152) for key-frame row kf_row on the resident map: cull_map_points ->
    api.map_remove(rm_mp, the count on the device).  -> dict(cull: the dict of cull_map_points, remove: the dict of api.map_remove - the
    edited map / ba, dead_mp for the host's mappoints_.erase).  Nothing is read back here (api.map_remove reads its 12 bytes)."""
    from .api import map_remove
    cull = cull_map_points(ctx, map, ba, stats, kf_row)
    rem = map_remove(ctx, map, ba, rm_mp=cull["rm_mp"], n_rm_mp=cull["n_rm"], mp_ref_kf=mp_ref_kf, want_new_pos=want_new_pos)
    return dict(cull=cull, remove=rem)
