"""GMMLoc::createMapPointsFromStereo (gmmloc_opt.cpp:36-113) and Tracking::createTemporalPoints (tracking.cpp:411-465) as sequential
Python, statement for statement, with the outputs named and shaped as gl_create_stereo_points / gl_create_temporal_points write them for
ONE key-frame / frame.  Test infrastructure: the model the device is held to (tests/test_gpu_key_frame_create.py), itself held to the
hand-declared outputs of tests/key_frame_create_cases.py (tests/test_key_frame_create_ref.py).

checkMapAssociation is a parameter: check(i, pt) -> (component or -1, the point as the check leaves it).  check_with(backend, ...) makes
one from the C++ oracle or oracle/numpy_ref.py, check_table(comp, pts) one from per-feature results computed elsewhere (the device's)."""
import numpy as np

f32, f64 = np.float32, np.float64


def _qrot(q, v):
    """Eigen's Quaternion::_transformVector, operation for operation"""
    x, y, z, w = q
    u = np.array([y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]], f64)
    u = u + u
    return np.array([v[0] + w * u[0] + (y * u[2] - z * u[1]), v[1] + w * u[1] + (z * u[0] - x * u[2]), v[2] + w * u[2] + (x * u[1] - y * u[0])], f64)


def twc_of(pose7):
    """SE3Quat(q, t) normalised as the constructor does, then SE3Quat::inverse -> (q, t) of Twc"""
    q = np.array(pose7[:4], f64)
    if q[3] < 0:
        q = -q
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qi = np.array([-q[0], -q[1], -q[2], q[3]], f64)
    return qi, _qrot(qi, -np.array(pose7[4:7], f64))


def unproject(cam, pose7, uv, depth):
    """Frame::unproject3 (frame.cpp:27-35): PinholeCamera::unproject3 (pinhole_camera.cpp:30-32: z (u - cx) / fx, z the float depth
    widened to double) then Twc.map.  cam: a dict with fx fy cx cy."""
    with np.errstate(invalid="ignore", over="ignore"):
        z = f64(f32(depth))
        ptc = np.array([z * (f64(uv[0]) - cam["cx"]) / cam["fx"], z * (f64(uv[1]) - cam["cy"]) / cam["fy"], z], f64)
        q, t = twc_of(pose7)
        return _qrot(q, ptc) + t


def _entries(fr):
    """(:37-44) the slots with z > 0 as a float compare; a slot whose octave is outside 0..7 is padding (gmmloc_hip.h) -> sorted (:49)"""
    e = []
    for i in range(len(fr["feat_depth"])):
        z = f32(fr["feat_depth"][i])
        if z > f32(0) and 0 <= int(fr["feat_oct"][i]) <= 7:
            e.append((z, i))
    e.sort()  # std::sort on pair<float, size_t>: by depth, then by index
    return e


def stereo_walk(cam, fr, check, mp_base, check_depth, th_depth, kf_row, pts0=None):
    """fr: pose (7,), feat_uv (NF,2), feat_ur / feat_depth (NF,) f32, feat_oct (NF,), cand (NF,k), ncand (NF,), held (NF,) -> dict of the
    outputs of gl_create_stereo_points for this key-frame; the lists hold n_new entries.  pts0 (NF,3): the unprojected points computed
    elsewhere (the device's, for a comparison of bits) instead of this file's"""
    NF = len(fr["feat_depth"])
    th_depth = f32(th_depth)
    entries = _entries(fr)
    if pts0 is None:
        pts0 = np.zeros((NF, 3), f64)
        for z, i in entries:
            pts0[i] = unproject(cam, fr["pose"], fr["feat_uv"][i], z)
    feat_new = -np.ones(NF, np.int32)
    new_feat, new_pos, new_assoc = [], [], []
    num_points = walked = rejected = broke = 0
    for z, i in entries:
        walked += 1
        create_new = False
        h = int(fr["held"][i])
        if h == 0:                       # if (!mappt)
            create_new = True
        elif h == 2:                     # else if (mappt->countObservations() < 1)
            create_new = True
            feat_new[i] = -2             #   frame->mappoints_[i] = nullptr
        if create_new:
            pt3d = pts0[i].copy()
            comp = -1
            if int(fr["ncand"][i]) > 0:  # if (!comps.empty())
                comp, pt3d = check(i, pt3d)
                if comp < 0:             #   if (!str_ptr) continue;
                    rejected += 1
                    continue
            feat_new[i] = len(new_feat)  # frame->mappoints_[i] = mappt
            new_feat.append(i)
            new_pos.append(np.array(pt3d, f64))
            new_assoc.append(int(comp))
            num_points += 1
        else:
            num_points += 1
        if check_depth and z > th_depth and num_points > 100:
            broke = 1
            break
    n = len(new_feat)
    i32 = lambda a: np.array(a, np.int32).reshape(-1)
    return dict(pts0=pts0, new_feat=i32(new_feat), new_pos=np.array(new_pos, f64).reshape(-1, 3), new_assoc=i32(new_assoc),
                new_ref_kf=i32([kf_row] * n), att_mp=i32([mp_base + r for r in range(n)]), att_kf=i32([kf_row] * n), att_feat=i32(new_feat),
                n_new=n, feat_new=feat_new, stats=i32([len(entries), walked, n, rejected, num_points, broke, 0, 0]))


def temporal_walk(cam, fr, last, th_depth):
    """fr: pose, feat_uv, feat_depth, feat_oct, held, last_outlier (NF,) u8, feat_desc (NF,32) u8; last: last_pt (NF,3), last_observed,
    last_valid (NF,) u8, last_desc (NF,32) u8 as the host wrote them -> dict(temp_flag, n_temp, stats, and the four arrays after the call)"""
    NF = len(fr["feat_depth"])
    th_depth = f32(th_depth)
    out = {k: np.array(v).copy() for k, v in last.items()}
    temp_flag = np.zeros(NF, np.uint8)
    entries = _entries(fr)
    num_pts = walked = broke = 0
    for z, i in entries:
        walked += 1
        if int(fr["held"][i]) != 1:      # !mappt, or countObservations() < 1: a new point takes the slot (:453)
            out["last_pt"][i] = unproject(cam, fr["pose"], fr["feat_uv"][i], z)
            out["last_observed"][i] = 0
            out["last_valid"][i] = 0 if fr["last_outlier"][i] else 1
            out["last_desc"][i] = fr["feat_desc"][i]
            temp_flag[i] = 1
            num_pts += 1
        else:
            num_pts += 1
        if z > th_depth and num_pts > 100:
            broke = 1
            break
    n = int(temp_flag.sum())
    return dict(out, temp_flag=temp_flag, n_temp=n, stats=np.array([len(entries), walked, n, 0, num_pts, broke, 0, 0], np.int32))


def check_table(comp, pts):
    """per-feature results computed elsewhere: comp (NF,), pts (NF,3) the points after the check"""
    return lambda i, pt: (int(comp[i]), np.array(pts[i], f64))


def check_with(ref, cam, fr):
    """ref: a tests.keyframe_cases.Ref (the C++ oracle's or numpy_ref's map)"""
    def check(i, pt):
        uvr = np.array([[fr["feat_uv"][i][0], fr["feat_uv"][i][1], f64(fr["feat_ur"][i])]], f64)
        out, p = ref.cma(cam, np.array(fr["pose"], f64), np.array(pt, f64)[None].copy(), uvr, np.array([fr["feat_oct"][i]], np.int32),
                         np.ascontiguousarray(fr["cand"][i][None], np.int32), np.array([fr["ncand"][i]], np.int32))
        return int(out[0]), np.array(p[0], f64)
    return check
