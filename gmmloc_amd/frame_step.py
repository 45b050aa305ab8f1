"""Frame end and hand-over on the device: gl_track_frame_end (the tail of Tracking::track + GMMLoc::needNewKeyFrame),
gl_map_note_replaced (ptr_replaced_ as a device array) and gl_track_frame_next (Map::updateFrameInfo, the pose block of
GMMLoc::processFrame, Tracking::updateLastFrame and the next last-frame rows); rules in include/gmmloc_hip.h.  track_frame_step is one
non-key frame from the chain call to the inputs of the next one.  Every wrapper only enqueues: what it returns are device tensors,
nothing is read back."""
import ctypes as C

from . import _lib
from ._host import _count, _map_ba_view, _map_view, _outputs, _ptr, _tensor

KF_NEED, KF_INTERRUPT_BA = 1, 2  # GL_KF_*
FRAME_NEXT_BAD_REF = 1           # GL_FRAME_NEXT_BAD_REF
MAX_NF = 3072
STAT_FIELDS = ("res", "num_match_inliers", "num_map", "num_total", "num_ref_matches", "verdict")
FRAME_KEYS = ("feat_uv", "feat_ur", "feat_oct", "feat_angle", "feat_desc", "feat_taken", "feat_depth")
STATE_KEYS = ("pose_lw", "pose_cw", "last_pt", "last_valid", "last_observed", "last_oct", "last_angle", "last_desc", "last_mp", "lists", "first")


def kf_rule(num_kfs, frame_idx, kf_frame_idx, fps, is_idle, n_queue):
    """the host scalars of GMMLoc::needNewKeyFrame (gmmloc.cpp:324-364) as a gl_kf_rule"""
    r = _lib.gl_kf_rule()
    r.num_kfs, r.frame_idx, r.kf_frame_idx, r.fps, r.is_idle, r.n_queue = int(num_kfs), int(frame_idx), int(kf_frame_idx), float(fps), int(bool(is_idle)), int(n_queue)
    return r


def frame_end(ctx, map, ba, chain, lm, feat_depth, th_depth, NL=None, last_observed=None, rule=None, out=None):
    """gl_track_frame_end for B frames.  chain: the dict api.track_frame_chain_map returned (feat_mp, match_last, match_local, outlier,
    counts2[, match_kf]); lm: the dict it was given (local_mp, n_local_mp, ref_kf as it left them); feat_depth (B,NF) f32;
    last_observed (B,NL) u8 or None; rule: a gl_kf_rule (kf_rule(...)) or None; map / ba: the dicts of api.map_remove (ba: kf_uvr,
    obs_feat - read with a rule only).  -> dict(held_mp (B,NF) i32, held (B,NF) u8, stat (B,8) i32, ratio_map (B,) f32); out: the dict
    of an earlier call, used again (a lost frame keeps its rows)."""
    v, dev = _map_view(map, False)
    B, NF = _tensor("chain['feat_mp']", chain.get("feat_mp"), "int32", (None, None), dev).shape
    assert NF <= MAX_NF, "NF %d above %d" % (NF, MAX_NF)
    i = _lib.gl_frame_end_in()
    for k, dt in (("feat_mp", "int32"), ("match_local", "int32"), ("outlier", "uint8")):
        setattr(i, k, _ptr(_tensor("chain[%r]" % k, chain.get(k), dt, (B, NF), dev)))
    for k in ("match_last", "match_kf"):  # (part of the C call for the header's statement on temporal points; no output depends on them)
        if chain.get(k) is not None:
            setattr(i, k, _ptr(_tensor("chain[%r]" % k, chain[k], "int32", (B, NF), dev)))
    if chain.get("counts2") is not None:
        i.counts2 = _ptr(_tensor("chain['counts2']", chain["counts2"], "int32", (B, 4), dev))
    NPcap = _tensor("lm['local_mp']", lm.get("local_mp"), "int32", (B, None), dev).shape[1]
    i.local_mp = _ptr(lm["local_mp"])
    i.n_local_mp = _ptr(_tensor("lm['n_local_mp']", lm.get("n_local_mp"), "int32", (B,), dev))
    if lm.get("ref_kf") is not None:
        i.ref_kf = _ptr(_tensor("lm['ref_kf']", lm["ref_kf"], "int32", (B,), dev))
    if last_observed is not None:
        NL = _tensor("last_observed", last_observed, "uint8", (B, None), dev).shape[1]
        i.last_observed = _ptr(last_observed)
    NL = NF if NL is None else int(NL)
    i.feat_depth = _ptr(_tensor("feat_depth", feat_depth, "float32", (B, NF), dev))
    w = None
    if rule is not None:
        assert isinstance(rule, _lib.gl_kf_rule), "rule: a gl_kf_rule (frame_step.kf_rule)"
        assert lm.get("ref_kf") is not None, "lm['ref_kf']: missing"
        w = _map_ba_view(ba, v, dev, need=("kf_uvr", "obs_feat"))
    out = _outputs(out, dict(held_mp=("int32", (B, NF), -1), held=("uint8", (B, NF), 0), stat=("int32", (B, 8), 0), ratio_map=("float32", (B,), 0)), dev)
    o = _lib.gl_frame_end_out()
    for k in ("held_mp", "held", "stat", "ratio_map"):
        setattr(o, k, _ptr(out[k]))
    ctx.call(ctx.lib.gl_track_frame_end, C.byref(v), C.byref(w) if w is not None else None, B, NF, NL, NPcap, C.byref(i), float(th_depth),
             C.byref(rule) if rule is not None else None, C.byref(o))
    return out


def note_replaced(ctx, mp_replaced, repl_src, repl_tgt, n=None, n_dev=None):
    """gl_map_note_replaced: mp_replaced (NMPcap,) i32 IN PLACE (-1 = none) from repl_src / repl_tgt of map_fuse in step order; n
    defaults to the tensors' length, n_dev (1,) i32 clamps it (result[3] of gl_map_fuse)."""
    NMPcap = _tensor("mp_replaced", mp_replaced, "int32", (None,), None).shape[0]
    dev = mp_replaced.device
    cap = _tensor("repl_src", repl_src, "int32", (None,), dev).shape[0]
    _tensor("repl_tgt", repl_tgt, "int32", (cap,), dev)
    n = cap if n is None else int(n)
    assert 0 <= n <= cap, "n %d outside [0, %d]" % (n, cap)
    ctx.call(ctx.lib.gl_map_note_replaced, NMPcap, _ptr(mp_replaced), _ptr(repl_src), _ptr(repl_tgt), n, _count("n_dev", n_dev, dev))


def frame_next(ctx, map, ba, pose_tracked, pose_prev, ref_kf, held_mp, feat_new=None, mp_base=0, mp_replaced=None, want_desc=False, out=None):
    """gl_track_frame_next for B frames on the map as it is NOW.  pose_tracked (B,7) f64; pose_prev (B,7) or None (no frame before);
    ref_kf (B,) i32; held_mp (B,NF) i32 IN/OUT; feat_new (B,NF) i32 + mp_base (of create_stereo_points) or None; mp_replaced (NMPcap,)
    i32 or None; map: obs_ptr, obs_kf, kf_mp, mp_pos (+ mp_desc with want_desc); ba: kf_pose.  -> dict(t_rc, t_cr, pose_lw, pose_cw
    (B,7) f64, held_mp (the tensor passed in), last_pt (B,NF,3) f64, last_valid / last_observed / held (B,NF) u8, status (B,) i32[,
    last_desc (B,NF,32) u8: the rows' map-point descriptors, zeros elsewhere]); out: the dict of an earlier call, used again."""
    v, dev = _map_view(map, False)
    assert v.NMP == 0 or map.get("mp_pos") is not None, "map['mp_pos']: missing"
    w = _map_ba_view(ba, v, dev, need=("kf_pose",))
    B, NF = _tensor("held_mp", held_mp, "int32", (None, None), dev).shape
    assert NF <= MAX_NF, "NF %d above %d" % (NF, MAX_NF)
    i = _lib.gl_frame_next_in()
    i.pose_tracked = _ptr(_tensor("pose_tracked", pose_tracked, "float64", (B, 7), dev))
    if pose_prev is not None:
        i.pose_prev = _ptr(_tensor("pose_prev", pose_prev, "float64", (B, 7), dev))
    i.ref_kf = _ptr(_tensor("ref_kf", ref_kf, "int32", (B,), dev))
    if feat_new is not None:
        i.feat_new = _ptr(_tensor("feat_new", feat_new, "int32", (B, NF), dev))
        i.mp_base = int(mp_base)
    if mp_replaced is not None:
        i.NMPcap = _tensor("mp_replaced", mp_replaced, "int32", (None,), dev).shape[0]
        assert i.NMPcap >= v.NMP, "mp_replaced has %d rows, the map %d" % (i.NMPcap, v.NMP)
        i.mp_replaced = _ptr(mp_replaced)
    spec = {k: ("float64", (B, 7), 0) for k in ("t_rc", "t_cr", "pose_lw", "pose_cw")}
    spec.update(last_pt=("float64", (B, NF, 3), 0), last_valid=("uint8", (B, NF), 0), last_observed=("uint8", (B, NF), 0), held=("uint8", (B, NF), 0),
                status=("int32", (B,), 0))
    if want_desc if out is None else out.get("last_desc") is not None:  # (optional: an `out` without it gets none)
        assert v.NMP == 0 or map.get("mp_desc") is not None, "map['mp_desc']: missing"
        spec["last_desc"] = ("uint8", (B, NF, 32), 0)
    out = _outputs(out, spec, dev)
    out["held_mp"] = held_mp  # (the caller's tensor, checked above)
    o = _lib.gl_frame_next_out()
    for k in (*spec, "held_mp"):
        setattr(o, k, _ptr(out[k]))
    ctx.call(ctx.lib.gl_track_frame_next, C.byref(v), C.byref(w), B, NF, C.byref(i), C.byref(o))
    return out


def first_state(a, last_mp, lists):
    """the state of track_frame_step before the first frame: the chain's last-frame inputs of `a` (pose_lw, pose_cw, last_pt,
    last_valid, last_oct, last_angle, last_desc[, last_observed]), last_mp (B,NL) i32 and the lists of api.local_map_lists; no frame
    before the last one (gl_track_frame_next gets no pose_prev)"""
    s = {k: a.get(k) for k in STATE_KEYS[:8]}
    s.update(last_mp=last_mp, lists=lists, first=True)
    return s


def track_frame_begin(ctx, cam, prm, state, frame, map, ba, stats, th_depth, rule=None, **kw):
    """The first half of track_frame_step, up to the key-frame decision: map_stats.track_frame_with_stats -> frame_end.  -> dict(chain,
    end, lm: the lists as the chain left them + last_mp).  A host that makes the frame a key-frame, or whose mapping pass has finished,
    applies it to the map now and calls track_frame_finish with what the pass reported."""
    from .map_stats import track_frame_with_stats
    for k in state:
        assert k in STATE_KEYS, "state[%r]: unknown key" % k
    for k in frame:
        assert k in FRAME_KEYS, "frame[%r]: unknown key" % k
    a = {k: frame[k] for k in FRAME_KEYS if k != "feat_depth"}
    a.update({k: state[k] for k in STATE_KEYS[:8] if state.get(k) is not None})
    lm = dict(state["lists"], last_mp=state["last_mp"])
    chain = track_frame_with_stats(ctx, cam, prm, a, map, lm, stats, **kw)
    end = frame_end(ctx, map, ba, chain, lm, frame["feat_depth"], th_depth, NL=state["last_mp"].shape[1], last_observed=state.get("last_observed"),
                    rule=rule)
    return dict(chain=chain, end=end, lm=lm)


def track_frame_finish(ctx, cam, state, frame, map, ba, begun, th_depth, feat_new=None, mp_base=0, mp_replaced=None, is_key_frame=False):
    """The second half: frame_next on the map as it is NOW (feat_new / mp_base of create_stereo_points and mp_replaced of note_replaced
    when a pass ran; lm['ref_kf'] as the host left it) -> key_frame.create_temporal_points on the rows it wrote, unless the frame has
    become a key-frame (tracking.cpp:44); a slot it replaces - a row that has lost its observations since the frame's end, or one step
    of mp_replaced onto a row that was itself replaced or culled - gets last_mp = -1 there, so that frame t + 1 matches it as a temporal
    point.  -> (the state for the next frame, dict(next, temporal or None))."""
    from .key_frame import create_temporal_points
    chain, end, lm = begun["chain"], begun["end"], begun["lm"]
    nxt = frame_next(ctx, map, ba, chain["pose"], None if state.get("first") else state["pose_lw"], lm["ref_kf"], end["held_mp"], feat_new=feat_new,
                     mp_base=mp_base, mp_replaced=mp_replaced, want_desc=True)
    last = {k: nxt[k] for k in ("last_pt", "last_observed", "last_valid", "last_desc")}
    tmp = None
    if not is_key_frame:  # (a held == 2 slot it replaces holds the temporal point from here on, tracking.cpp:453: its last_mp becomes -1)
        tmp = create_temporal_points(ctx, cam, dict(pose=nxt["pose_lw"], feat_uv=frame["feat_uv"], feat_depth=frame["feat_depth"], feat_oct=frame["feat_oct"],
                                                    held=nxt["held"], last_outlier=chain["outlier"], feat_desc=frame["feat_desc"]), last, th_depth,
                                     last_mp=nxt["held_mp"])
    new = dict(last, pose_lw=nxt["pose_lw"], pose_cw=nxt["pose_cw"], last_oct=frame["feat_oct"], last_angle=frame["feat_angle"], last_mp=nxt["held_mp"],
               lists=state["lists"], first=False)
    return new, dict(next=nxt, temporal=tmp)


def track_frame_step(ctx, cam, prm, state, frame, map, ba, stats, th_depth, rule=None, **kw):
    """One non-key frame, from the chain call to the inputs of the next one, enqueued with no synchronise in between:
    map_stats.track_frame_with_stats -> frame_end -> frame_next -> key_frame.create_temporal_points on the rows it wrote
    (track_frame_begin + track_frame_finish).
    state: first_state(...) or the state an earlier call returned; frame: the frame's feature buffers (FRAME_KEYS; feat_depth (B,NF)
    f32); map / ba / stats: the resident map (api.track_frame_chain_map's map with mp_desc; ba: kf_pose, kf_uvr, obs_feat) and its
    counters; kw: th_mm / th_local / nn_ratio / mono / scale_factor of the chain.
    -> (the state for the next frame - the frame's feature buffers are its last_oct / last_angle, no copy -, dict(chain, end, next,
    temporal): each call's device tensors; end['stat'] (B,8) i32 stays on the device).
    A LOST frame (counts2[3] == 2) is not handled on the device: frame_end writes only its stat, so the state returned for it is built
    from empty rows and the lost frame's pose, and every frame enqueued behind it runs on that.  In the reference last_frame_ does not
    advance (tracking.cpp:65-71).  No call writes into the poses or last-frame rows of the state it was given (only `lists`, the chain's
    in/out buffers, are shared), so a host that enqueues frames back to back keeps the states it passed in until it has read counts2
    (or stat: res 0 with num_match_inliers 10), and on a lost frame goes on from the state that frame was GIVEN and drops what was
    enqueued behind it."""
    begun = track_frame_begin(ctx, cam, prm, state, frame, map, ba, stats, th_depth, rule=rule, **kw)
    new, r = track_frame_finish(ctx, cam, state, frame, map, ba, begun, th_depth)
    return new, dict(chain=begun["chain"], end=begun["end"], **r)
