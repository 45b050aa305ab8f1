"""The sequential model of gl_create_map_points_from_map: Localization::createMapPoints (localization_opt.cpp:206-454) as a Python loop over
the neighbours, with a callable for searchForTriangulation, for the per-match block and for the fundamental matrix / epipole.  has_mp1 is
updated per created point (curr_kf_->addObservation(mappt, idx1), :433), the lists come out in creation order.  Test infrastructure.

A scene is three dicts of numpy arrays, row-indexed like the device's: map (kf_valid, kf_mp[, the CSR and the per-point arrays]), ba
(kf_pose, kf_twc, kf_uvr, kf_oct) and kt (angle, desc, depth, nnode, node_id, node_ptr, node_idx, cand, ncand)."""
import numpy as np

f32, f64 = np.float32, np.float64
SKIP_BEYOND, SKIP_BAD_ROW, SKIP_SELF, SKIP_INVALID, SKIP_REPEATED, SKIP_BASELINE = 1, 2, 4, 8, 16, 32
NONE_SEARCHED = 1
LIST_KEYS = ("new_assoc", "new_ref_kf", "new_type", "new_nb", "new_feat1", "new_feat2")
ATT_KEYS = ("att_mp", "att_kf", "att_feat")


def cam_scalars(cam):
    """the camera's float config scalars, widened"""
    g = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
    return tuple(float(f32(g(k))) for k in ("fx", "fy", "cx", "cy"))


def _qrot(q, v):  # Eigen's _transformVector
    x, y, z, w = q
    ux, uy, uz = y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return (v[0] + w * ux + (y * uz - z * uy), v[1] + w * uy + (z * ux - x * uz), v[2] + w * uz + (x * uy - y * ux))


def _qtoR(q):  # Eigen's toRotationMatrix
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def fundamental_and_epipole(pose1, pose2, cam):
    """The numpy statement of the device's declared expression order (gmmloc_hip.h, gl_tri_pair_setup): Python floats are IEEE doubles
    and nothing is contracted, so this gives the device's bits.  -> (F (9,) f64 row-major, epipole (2,) f32)"""
    fx, fy, cx, cy = cam_scalars(cam)
    p1, p2 = [float(v) for v in pose1], [float(v) for v in pose2]
    R1, R2 = _qtoR(p1[:4]), _qtoR(p2[:4])
    R = [[(R1[i][0] * R2[j][0] + R1[i][1] * R2[j][1]) + R1[i][2] * R2[j][2] for j in range(3)] for i in range(3)]
    r = [(R[i][0] * p2[4] + R[i][1] * p2[5]) + R[i][2] * p2[6] for i in range(3)]
    tx, ty, tz = -r[0] + p1[4], -r[1] + p1[5], -r[2] + p1[6]
    E = [[(-tz) * R[1][j] + ty * R[2][j] for j in range(3)], [tz * R[0][j] + (-tx) * R[2][j] for j in range(3)],
         [(-ty) * R[0][j] + tx * R[1][j] for j in range(3)]]
    ifx, ify, mcx, mcy = 1.0 / fx, 1.0 / fy, -(cx / fx), -(cy / fy)
    G = [[E[i][0] * ifx, E[i][1] * ify, (E[i][0] * mcx + E[i][1] * mcy) + E[i][2]] for i in range(3)]
    F = [ifx * G[0][j] for j in range(3)] + [ify * G[1][j] for j in range(3)] + [(mcx * G[0][j] + mcy * G[1][j]) + G[2][j] for j in range(3)]
    c = _qrot(p2[:4], p1[4:])
    c0, c1, c2 = c[0] + p2[4], c[1] + p2[5], c[2] + p2[6]
    with np.errstate(all="ignore"):
        invz = f32(1.0) / f32(c2)
        e = np.array([f32(f64(fx * c0) * f64(invz) + cx), f32(f64(fy * c1) * f64(invz) + cy)], f32)
    return np.array(F, f64), e


def pair_setup(cam, kf_valid, kf_pose, kf_twc, kf_row, conn_kf, n_conn, first_nb, n_nb, mb, fe=fundamental_and_epipole):
    """-> skip (n_nb,) i32, rows (n_nb,) i32 (-1 beyond the list), fmat (n_nb, 9), epipole (n_nb, 2); zeros for a skipped neighbour"""
    NKF = len(kf_pose)
    length = min(max(int(n_conn), 0), len(conn_kf))
    skip, rows = np.zeros(n_nb, np.int32), -np.ones(n_nb, np.int32)
    fmat, epi = np.zeros((n_nb, 9), f64), np.zeros((n_nb, 2), f32)
    for j in range(n_nb):
        i = first_nb + j
        if i >= length:
            skip[j] = SKIP_BEYOND
            continue
        row = rows[j] = int(conn_kf[i])
        if row < 0 or row >= NKF:
            skip[j] = SKIP_BAD_ROW
            continue
        bits = 0
        if row == kf_row:
            bits |= SKIP_SELF
        if kf_valid is not None and not kf_valid[row]:
            bits |= SKIP_INVALID
        if any(int(conn_kf[e]) == row for e in range(first_nb, i)):
            bits |= SKIP_REPEATED
        d = [float(kf_twc[row][c]) - float(kf_twc[kf_row][c]) for c in range(3)]
        baseline = f32(np.sqrt(f64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
        if baseline < f32(mb):
            bits |= SKIP_BASELINE
        skip[j] = bits
        if bits == 0:
            fmat[j], epi[j] = fe(kf_pose[kf_row], kf_pose[row], cam)
    return skip, rows, fmat, epi


def kf_side(ba, kt, row, has_mp):
    """key-frame `row` as the dict search_for_triangulation takes (oracle_lib / numpy_ref: the CSR cut to the nodes in use)"""
    nn = int(kt["nnode"][row])
    uvr = ba["kf_uvr"][row]
    return dict(row=row, uv=np.ascontiguousarray(uvr[:, :2]), ur=uvr[:, 2].astype(f32), oct=ba["kf_oct"][row], angle=kt["angle"][row], desc=kt["desc"][row],
                has_mp=np.asarray(has_mp, np.uint8), node_id=kt["node_id"][row][:nn], node_ptr=kt["node_ptr"][row][:nn + 1], node_idx=kt["node_idx"][row])


def match_arrays(ba, kt, kf_row, kf2, match):
    """the per-match arrays of the matches of one pair in ascending idx1 (= matched_pairs) -> (dict, idx1, idx2)"""
    i1 = np.nonzero(match >= 0)[0].astype(np.int32)
    i2 = match[i1].astype(np.int32)
    n = len(i1)
    u1, u2 = ba["kf_uvr"][kf_row][i1], ba["kf_uvr"][kf2][i2]
    uvr = lambda u: np.concatenate([u[:, :2], u[:, 2].astype(f32).astype(f64)[:, None]], 1).reshape(n, 3)
    a = dict(pose1=np.tile(ba["kf_pose"][kf_row], (n, 1)), uvr1=uvr(u1), depth1=kt["depth"][kf_row][i1], oct1=ba["kf_oct"][kf_row][i1],
             pose2=np.tile(ba["kf_pose"][kf2], (n, 1)), uvr2=uvr(u2), depth2=kt["depth"][kf2][i2], oct2=ba["kf_oct"][kf2][i2],
             cand1=kt["cand"][kf_row][i1], n1=kt["ncand"][kf_row][i1], cand2=kt["cand"][kf2][i2], n2=kt["ncand"][kf2][i2])
    return a, i1, i2


def create_points(cam, map, ba, kt, kf_row, conn_kf, n_conn, first_nb, n_nb, mb, mp_base, search, create, fe=fundamental_and_epipole, pairs=None,
                  carry=True, gather=None):
    """Localization::createMapPoints for key-frame row kf_row over conn_kf[first_nb .. first_nb + n_nb).
    search(kf1, kf2, fmat, epipole) -> match12; create(**per-match arrays) -> (x3d, type, comp).  pairs: (skip, rows, fmat, epipole) to use
    instead of pair_setup's (the device's own); gather(kf2, match) -> (per-match arrays, idx1, idx2) instead of match_arrays.  carry = False: the mask is NOT updated (what a batch of independent pairs would give).
    -> dict of every output of the device call, the lists cut to n_new / n_attach."""
    NFK = map["kf_mp"].shape[1]
    skip, rows, fmat, epi = pairs if pairs is not None else pair_setup(cam, map.get("kf_valid"), ba["kf_pose"], ba["kf_twc"], kf_row, conn_kf, n_conn,
                                                                      first_nb, n_nb, mb, fe)
    has_mp1 = (map["kf_mp"][kf_row] != -1).astype(np.uint8)
    feat_new = -np.ones(NFK, np.int32)
    out = {k: [] for k in LIST_KEYS + ATT_KEYS}
    pos = []
    stats = np.zeros((n_nb, 8), np.int32)
    for j in range(n_nb):
        stats[j, :2] = rows[j], skip[j]
        if skip[j]:
            continue
        kf2 = int(rows[j])
        match = np.asarray(search(kf_side(ba, kt, kf_row, has_mp1), kf_side(ba, kt, kf2, map["kf_mp"][kf2] != -1), fmat[j], epi[j]), np.int32)
        a, i1, i2 = gather(kf2, match) if gather else match_arrays(ba, kt, kf_row, kf2, match)
        stats[j, 2] = len(i1)
        if len(i1) == 0:
            continue
        x3d, typ, comp = create(**a)
        for m in range(len(i1)):
            if typ[m] <= 0:
                stats[j, 4] += 1
                continue
            r = len(pos)
            pos.append(np.array(x3d[m], f64))
            for k, v in zip(LIST_KEYS, (comp[m], kf_row, typ[m], first_nb + j, i1[m], i2[m])):
                out[k].append(int(v))
            out["att_mp"] += [mp_base + r, mp_base + r]
            out["att_kf"] += [kf_row, kf2]
            out["att_feat"] += [int(i1[m]), int(i2[m])]
            if carry:
                has_mp1[i1[m]] = 1
            feat_new[i1[m]] = mp_base + r
            stats[j, 3] += 1
    res = {k: np.array(v, np.int32) for k, v in out.items()}
    res.update(new_pos=np.array(pos, f64).reshape(-1, 3), n_new=len(pos), n_attach=2 * len(pos), feat_new=feat_new, nb_stats=stats, skip=skip, fmat=fmat,
               epipole=epi, status=NONE_SEARCHED if not (skip == 0).any() else 0)
    return res
