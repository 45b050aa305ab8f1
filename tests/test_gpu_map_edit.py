"""gl_cull_keyframes and gl_map_remove against the sequential object model of tests/map_edit_ref.py - integers and float compares, so
equality is exact and every entry behind an output's contents must keep its sentinel - the readers of the resident map on the
device-edited arrays, and the mapping pass (api.mapping_pass_from_map) against the same pass with the edits made on the host.  The
scenes and the conditions they meet: tests/map_edit_scenes.py, tests/test_map_edit_ref.py."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import map_edit_ref as E
from tests import map_edit_scenes as ES
from tests import map_point_ref as M
from tests.gpu_helpers import to_dev
from tests.test_gpu_ba_window import to_host

pytestmark = pytest.mark.gpu

CULL_KEYS = ("cull", "num_mps", "num_redundant", "cand_status", "cull_rows", "n_cull")
MAP_KEYS = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr")
BIG = ("euroc", "kf_at_bound", "kf_over_bound")  # judged by the vectorised restatement (equal to the model: tests/test_map_edit_ref.py)


def same(dev, ref, what, keys):
    for k in keys:
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, np.nonzero((a != b).reshape(len(b), -1).any(1))[0][:8])


def cull_out(B, Ccap):
    out = {k: np.full((B, Ccap), 77 if k == "cull" else -7, api.CULL_DTYPES[k]) for k in api.CULL_DTYPES}
    out["n_cull"] = np.full(B, -7, np.int32)
    return out


def lists_of(sc, Ccap):
    """the candidate lists of a scene: its list, the same again, reversed, a short one, one with kf_first, an invalid row, a duplicate and
    rows outside the table in it"""
    m, ba, c = sc["m"], sc["ba"], sc["cand"]
    NKF = len(m["kf_valid"])
    bad = np.nonzero(m["kf_valid"] == 0)[0][:1]
    mixed = np.concatenate([c[:3], [ba["kf_first"], -1, NKF, 2 ** 31 - 1], bad, c[1:2], c[3:12]]).astype(np.int32)
    ls = [c, c, c[::-1], c[:5], mixed]
    cand = np.full((len(ls), Ccap), -3, np.int32)
    for b, l in enumerate(ls):
        cand[b, :len(l)] = l
    n = np.array([len(l) for l in ls], np.int32)
    n[3] = Ccap + 9  # a true length above the capacity, as gl_update_connections reports one: the first Ccap
    cand[3, 5:] = c[:1]  # (duplicates of its first entry)
    return cand, n


def device_cull(torch, ctx, md, bd, sc, cand, n_cand, out):
    od = to_dev(torch, out)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    api.cull_keyframes(ctx, md, bd, T(sc["kf_depth"]), sc["th_depth"], T(cand), T(n_cand), out=od)
    torch.cuda.synchronize()
    return to_host(od)


def by_state(sc):
    return lambda lst: E.cull_by_state(sc["m"], sc["ba"], lst, sc["kf_depth"], sc["th_depth"])


@pytest.mark.parametrize("name,clamp", [(n, False) for n in S.SMALL + BIG] + [(n, True) for n in ES.CLAMP])
def test_cull_keyframes_equals_the_restatement(gpu, name, clamp):
    """every output array of every list, the entries at and behind n_cand still holding their sentinels; the same list twice in a batch;
    the map's arrays bit-identical afterwards; twice the same bytes"""
    torch, ctx = gpu
    sc = ES.scene(name, clamp)
    Ccap = len(sc["cand"]) + 6
    cand, n_cand = lists_of(sc, Ccap)
    out = cull_out(len(cand), Ccap)
    ref = E.cull_keyframes(sc["m"], sc["ba"], cand, n_cand, sc["kf_depth"], sc["th_depth"], out, by_state(sc) if name in BIG else None)
    assert {E.JUDGED, E.FIRST, E.BAD_ROW, E.INVALID, E.DUPLICATE} <= set(ref["cand_status"][4].tolist())
    if clamp:
        assert ref["n_cull"][0] >= 3
    md, bd = to_dev(torch, sc["m"]), to_dev(torch, sc["ba"])
    dev = device_cull(torch, ctx, md, bd, sc, cand, n_cand, out)
    same(dev, ref, (name, clamp), CULL_KEYS)
    assert dev["cull"][0].tobytes() == dev["cull"][1].tobytes() and dev["cull_rows"][0].tobytes() == dev["cull_rows"][1].tobytes()
    for k, v in sc["m"].items():
        assert md[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), k
    for k in ("kf_uvr", "kf_oct", "obs_feat"):
        assert bd[k].cpu().numpy().tobytes() == np.ascontiguousarray(sc["ba"][k]).tobytes(), k
    again = device_cull(torch, ctx, md, bd, sc, cand, n_cand, out)
    assert all(again[k].tobytes() == dev[k].tobytes() for k in CULL_KEYS)


def test_cull_keyframes_takes_the_lists_of_update_connections(gpu):
    """conn_kf / n_conn straight from gl_update_connections on the device, one capacity below the longest list (its n_conn is the true
    length, above Ccap)"""
    torch, ctx = gpu
    sc = ES.scene("small", True)
    m, ba, rows = sc["m"], sc["ba"], sc["rows"]
    n = [len(R.connections_vec(m, int(kf))["conn_kf"]) for kf in rows]
    Ccap = max(n) - 1
    B = len(rows)
    conn = dict(conn_kf=np.full((B, Ccap), -7, np.int32), conn_w=np.full((B, Ccap), -7, np.int32), n_conn=np.full(B, -7, np.int32), status=np.full(B, -7, np.int32))
    cref = R.update_connections(m, rows, conn)
    assert (cref["n_conn"] > Ccap).any() and (cref["n_conn"] == 0).any()
    out = cull_out(B, Ccap)
    ref = E.cull_keyframes(m, ba, cref["conn_kf"], cref["n_conn"], sc["kf_depth"], sc["th_depth"], out)
    assert ref["cull"][ref["cull"] != 77].sum() >= 3
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    cd = api.update_connections(ctx, md, torch.from_numpy(rows).cuda(), out=to_dev(torch, conn))
    od = to_dev(torch, out)
    api.cull_keyframes(ctx, md, bd, torch.from_numpy(sc["kf_depth"]).cuda(), sc["th_depth"], cd["conn_kf"], cd["n_conn"], out=od)
    torch.cuda.synchronize()
    same(to_host(od), ref, "chained", CULL_KEYS)


@pytest.mark.parametrize("name", ["small", "kf_over_bound"])
def test_cull_keyframes_skips_malformed_input(gpu, name):
    """rows outside the tables in kf_mp, obs_kf and obs_feat, CSR ranges outside [0, NOBS]: skipped as gmmloc_hip.h says (the CSR decides
    what a key-frame observes: the restatement by state), every output exact behind its sentinels"""
    torch, ctx = gpu
    sc = ES.scene(name, name in ES.CLAMP)
    S.malform(sc["m"], sc["ba"], 5)
    Ccap = len(sc["cand"]) + 6
    cand, n_cand = lists_of(sc, Ccap)
    out = cull_out(len(cand), Ccap)
    ref = E.cull_keyframes(sc["m"], sc["ba"], cand, n_cand, sc["kf_depth"], sc["th_depth"], out, by_state(sc))
    assert (ref["num_mps"][0] > 0).any()
    dev = device_cull(torch, ctx, to_dev(torch, sc["m"]), to_dev(torch, sc["ba"]), sc, cand, n_cand, out)
    same(dev, ref, name, CULL_KEYS)


def test_cull_keyframes_bound_on_the_key_frames(gpu):
    """GL_CULL_MAX_KF key-frames run (the two bit sets fill 128 KB of LDS) and equal the restatement; one more is refused"""
    torch, ctx = gpu
    rng = np.random.default_rng(3)
    for NKF in (api.CULL_MAX_KF, api.CULL_MAX_KF + 1):
        NMP, NFK = 64, 1
        kf_mp = -np.ones((NKF, NFK), np.int32)
        obs = rng.choice(NKF, (NMP, 5), replace=False)  # five observers per point, every key-frame observes at most one point
        obs[:, 0] = NKF - 1 - np.arange(NMP)  # (the last rows are used: the top of the bit sets)
        obs[:, 1:] = rng.choice(NKF - NMP, (NMP, 4), replace=False)
        kf_mp[obs, 0] = np.arange(NMP)[:, None]
        m = dict(mp_valid=np.ones(NMP, np.uint8), kf_valid=np.ones(NKF, np.uint8), kf_mp=kf_mp, obs_ptr=(5 * np.arange(NMP + 1)).astype(np.int32),
                 obs_kf=obs.ravel().astype(np.int32))
        uvr = np.zeros((NKF, NFK, 3))
        uvr[:, :, 2] = 1.0
        ba = dict(kf_uvr=uvr, kf_oct=np.zeros((NKF, NFK), np.int32), obs_feat=np.zeros(5 * NMP, np.int32), kf_first=0)
        depth = np.ones((NKF, NFK), np.float32)
        cand = obs[:8, 0].astype(np.int32)[None]
        n_cand = np.array([8], np.int32)
        out = cull_out(1, 8)
        sc = dict(m=m, ba=ba, kf_depth=depth, th_depth=6.0)
        if NKF > api.CULL_MAX_KF:
            with pytest.raises(api.GLError, match="GL_CULL_MAX_KF"):
                device_cull(torch, ctx, to_dev(torch, m), to_dev(torch, ba), sc, cand, n_cand, out)
            continue
        ref = E.cull_keyframes(m, ba, cand, n_cand, depth, 6.0, out, by_state(sc))
        assert ref["n_cull"][0] == 8
        same(device_cull(torch, ctx, to_dev(torch, m), to_dev(torch, ba), sc, cand, n_cand, out), ref, NKF, CULL_KEYS)


# ---- gl_map_remove

def device_remove(torch, ctx, sc, rm_mp=None, erase=None, rm_kf=None, counts=False, md=None, bd=None, ref_kf=None, dead_cap=None):
    """-> (rows as Model.to_rows gives them + nobs, status, n_dead; the device dicts).  counts: the lengths as device ints, the lists
    padded behind them"""
    if md is None:
        md, bd = to_dev(torch, sc["m"]), to_dev(torch, sc["ba"])
        ref_kf = torch.from_numpy(sc["mp_ref_kf"].copy()).cuda()
    kw = {}
    for key, nkey, lst in (("rm_mp", "n_rm_mp", rm_mp), ("erase_obs", "n_erase", erase), ("rm_kf", "n_rm_kf", rm_kf)):
        if lst is None:
            continue
        lst = np.asarray(lst, np.int32)
        if counts:
            kw[nkey] = torch.tensor([len(lst)], dtype=torch.int32, device="cuda")
            lst = np.concatenate([lst, np.zeros(7, np.int32)])  # (row / position 0 behind the count: must not be read as an entry)
        kw[key] = torch.from_numpy(lst.copy()).cuda()
    NOBS = md["obs_kf"].shape[0]
    r = api.map_remove(ctx, md, bd, mp_ref_kf=ref_kf, want_new_pos=True, dead_cap=dead_cap, **kw)
    torch.cuda.synchronize()
    n = r["nobs"]
    rows = {k: md[k].cpu().numpy() for k in MAP_KEYS}
    rows.update(obs_kf=md["obs_kf"].cpu().numpy()[:n], obs_feat=bd["obs_feat"].cpu().numpy()[:n], mp_ref_kf=ref_kf.cpu().numpy(),
                obs_new_pos=r["obs_new_pos"].cpu().numpy(), dead_mp=r["dead_mp"].cpu().numpy(), nobs=n, status=r["status"], n_dead=r["n_dead"],
                tail_kf=md["obs_kf"].cpu().numpy()[n:], tail_feat=bd["obs_feat"].cpu().numpy()[n:])
    assert r["map"]["obs_kf"].shape[0] == n and r["ba"]["obs_feat"].shape[0] == n and r["map"]["obs_kf"].data_ptr() == md["obs_kf"].data_ptr()
    assert len(rows["obs_new_pos"]) == NOBS
    return rows, (md, bd, ref_kf)


ROW_KEYS = MAP_KEYS + ("obs_kf", "obs_feat", "mp_ref_kf", "obs_new_pos", "dead_mp")


def check_rows(dev, ref, status, sc, what):
    same(dev, ref, what, ROW_KEYS)
    n = len(ref["obs_kf"])
    assert dev["nobs"] == n == ref["obs_ptr"][-1] and dev["status"] == status and dev["n_dead"] == len(ref["dead_mp"]), what
    # the arrays behind the new NOBS are not written
    assert np.array_equal(dev["tail_kf"], sc["m"]["obs_kf"][n:]) and np.array_equal(dev["tail_feat"], sc["ba"]["obs_feat"][n:]), what


@pytest.mark.parametrize("kind", ["mp", "obs", "kf", "all", "dirty", "counted"])
@pytest.mark.parametrize("name", S.SMALL)
def test_map_remove_equals_the_restatement(gpu, name, kind):
    """all seven arrays up to the new NOBS (the removed key-frames' rows included), dead_mp, obs_new_pos, the new NOBS and the status: each
    kind of removal alone, the three together, lists with duplicates / invalid rows / rows outside the tables / kf_first, the lengths
    as device counts; a second identical call (points and key-frames: a CSR position means another entry by then) changes nothing"""
    torch, ctx = gpu
    sc = ES.scene(name, name in ES.CLAMP)
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    if kind == "dirty":
        rm_mp, erase, rm_kf = ES.dirty(sc, rm_mp, erase, rm_kf)
    use = dict(mp=(rm_mp, None, None), obs=(None, erase, None), kf=(None, None, rm_kf)).get(kind, (rm_mp, erase, rm_kf))
    e = lambda l: () if l is None else l
    ref, status = E.map_remove(sc["m"], sc["ba"], e(use[0]), e(use[1]), e(use[2]), sc["mp_ref_kf"])
    assert status == (E.FIRST_REFUSED if kind == "dirty" else 0)
    assert len(ref["dead_mp"]) > 0 and (kind == "mp" or len(ref["obs_kf"]) < len(sc["m"]["obs_kf"]))
    dev, (md, bd, ref_kf) = device_remove(torch, ctx, sc, *use, counts=kind == "counted")
    check_rows(dev, ref, status, sc, (name, kind))
    if kind in ("mp", "kf"):
        md2 = dict(md, obs_kf=md["obs_kf"][:dev["nobs"]])
        bd2 = dict(bd, obs_feat=bd["obs_feat"][:dev["nobs"]])
        again, _ = device_remove(torch, ctx, sc, *use, md=md2, bd=bd2, ref_kf=ref_kf)
        same(again, ref, (name, kind, "again"), MAP_KEYS + ("obs_kf", "obs_feat", "mp_ref_kf"))
        assert again["n_dead"] == 0 and again["nobs"] == dev["nobs"] and np.array_equal(again["obs_new_pos"], np.arange(dev["nobs"]))


def test_map_remove_in_the_reversed_order_follows_the_rank(gpu):
    """the removed key-frames' rows depend on the list order (fact 2): both orders equal the restatement, and they differ"""
    torch, ctx = gpu
    sc = ES.scene("small")
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    got = []
    for lst in (rm_kf, rm_kf[::-1].copy()):
        ref, status = E.map_remove(sc["m"], sc["ba"], rm_mp, erase, lst, sc["mp_ref_kf"])
        dev, _ = device_remove(torch, ctx, sc, rm_mp, erase, lst)
        check_rows(dev, ref, status, sc, "order")
        got.append(dev["kf_mp"])
    assert not np.array_equal(got[0], got[1])


def test_map_remove_of_nothing_changes_nothing(gpu):
    torch, ctx = gpu
    sc = ES.scene("small")
    none = np.zeros(0, np.int32)
    for use in ((None, None, None), (none, none, none)):
        dev, _ = device_remove(torch, ctx, sc, *use)
        for k in MAP_KEYS:
            assert dev[k].tobytes() == sc["m"][k].tobytes(), k
        assert dev["obs_kf"].tobytes() == sc["m"]["obs_kf"].tobytes() and dev["obs_feat"].tobytes() == sc["ba"]["obs_feat"].tobytes()
        assert dev["nobs"] == len(sc["m"]["obs_kf"]) and dev["n_dead"] == 0 and dev["status"] == 0 and np.array_equal(dev["mp_ref_kf"], sc["mp_ref_kf"])
        assert np.array_equal(dev["obs_new_pos"], np.arange(dev["nobs"]))
    dev, _ = device_remove(torch, ctx, sc, None, None, sc["cand"][:0], counts=True)  # a device count of 0
    assert dev["nobs"] == len(sc["m"]["obs_kf"]) and dev["kf_valid"].tobytes() == sc["m"]["kf_valid"].tobytes()


def test_map_remove_dead_capacity(gpu):
    """more deaths than dead_cap: the first dead_cap rows, the true count, the status bit"""
    torch, ctx = gpu
    sc = ES.scene("small")
    rm_mp, erase, rm_kf = ES.removals(sc, 3)
    ref, _ = E.map_remove(sc["m"], sc["ba"], rm_mp, erase, rm_kf, sc["mp_ref_kf"])
    cap = len(ref["dead_mp"]) - 3
    dev, _ = device_remove(torch, ctx, sc, rm_mp, erase, rm_kf, dead_cap=cap)
    assert dev["status"] == E.DEAD_TRUNCATED and dev["n_dead"] == len(ref["dead_mp"]) and np.array_equal(dev["dead_mp"], ref["dead_mp"][:cap])
    same(dev, ref, "dead_cap", MAP_KEYS + ("obs_kf", "obs_feat"))


def test_map_remove_above_2_20_map_points(gpu):
    """`mp_over_bound` (1 048 577 points: 257 tiles of the scan), the three kinds together"""
    torch, ctx = gpu
    sc = ES.scene("mp_over_bound")
    rm_mp, erase, rm_kf = ES.removals(sc, 3, n_mp=500, n_kf=40, erase_frac=0.01)
    ref, status = E.map_remove(sc["m"], sc["ba"], rm_mp, erase, rm_kf, sc["mp_ref_kf"])
    assert len(ref["dead_mp"]) > 500 and (ref["dead_mp"] > (1 << 20) - 4096).any()
    dev, _ = device_remove(torch, ctx, sc, rm_mp, erase, rm_kf)
    check_rows(dev, ref, status, sc, "mp_over_bound")


# ---- the readers on the edited map

def test_the_readers_take_the_edited_map(gpu):
    """gl_update_connections, gl_ba_window_build, gl_update_local_map and gl_update_map_points on the device-edited arrays (the CSR a view
    cut to the new NOBS) give bit for bit what they give on the restatement's edited map uploaded afresh"""
    torch, ctx = gpu
    sc = ES.scene("small", True)
    m, ba, rows = sc["m"], sc["ba"], sc["rows"]
    rm_mp, erase, _ = ES.removals(sc, 3)
    cull = E.Model(m, ba).remove_key_frames(sc["cand"], sc["kf_depth"], sc["th_depth"])
    ref, _ = E.map_remove(m, ba, rm_mp, erase, cull["cull_rows"], sc["mp_ref_kf"])
    m2, ba2 = E.apply_rows(m, ba, ref)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    ref_kf = torch.from_numpy(sc["mp_ref_kf"].copy()).cuda()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = api.map_remove(ctx, md, bd, erase_obs=T(erase), rm_kf=T(cull["cull_rows"]), rm_mp=T(rm_mp), mp_ref_kf=ref_kf)
    assert r["nobs"] == len(ref["obs_kf"]) < len(m["obs_kf"])
    fresh_m, fresh_b = to_dev(torch, m2), to_dev(torch, ba2)
    rw = torch.from_numpy(rows).cuda()
    outs = []
    for mm, bb, rk in ((r["map"], r["ba"], ref_kf), (fresh_m, fresh_b, T(ref["mp_ref_kf"]))):
        conn = api.update_connections(ctx, mm, rw, Ccap=64, want_count=True)
        _, wins = R.ba_window_build(m2, ba2, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
        slab = to_dev(torch, S.empty_slab(len(rows), S.caps_of(wins)))
        api.ba_window_build(ctx, mm, bb, rw, slab)
        NKF, NMP = len(m["kf_valid"]), len(m["mp_valid"])
        feat = mm["kf_mp"][rw.long()].clone()
        lists = api.local_map_lists(len(rows), 128, 4096, NKF, device="cuda")
        api.update_local_map(ctx, {k: mm[k] for k in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")}, feat, lists)
        od = to_dev(torch, dict(normal=np.full((NMP, 3), -7.0), max_dist=np.full(NMP, -1.0, np.float32), min_dist=np.full(NMP, -2.0, np.float32)))
        api.update_map_points(ctx, dict(twc=bb["kf_twc"], valid=mm["kf_valid"], oct=bb["kf_oct"]),
                              dict(pos=mm["mp_pos"], valid=mm["mp_valid"], ref_kf=rk, obs_ptr=mm["obs_ptr"], obs_kf=mm["obs_kf"], obs_feat=bb["obs_feat"]), od, what=2)
        torch.cuda.synchronize()
        outs.append(dict(conn=to_host(conn), slab=to_host(slab), feat=feat.cpu().numpy(), lists=to_host(lists), mp=to_host(od)))
    a, b = outs
    for grp in ("conn", "slab", "lists", "mp"):
        same(a[grp], b[grp], grp, list(b[grp]))
    assert a["feat"].tobytes() == b["feat"].tobytes()
    # ... and what they give is the restatement's answer on the edited map
    conn = R.update_connections(m2, rows, {k: np.zeros_like(v) - (k == "conn_kf") for k, v in b["conn"].items()})
    same(a["conn"], conn, "connections", list(conn))
    out = dict(normal=np.full((len(m["mp_valid"]), 3), -7.0), max_dist=np.full(len(m["mp_valid"]), -1.0, np.float32), min_dist=np.full(len(m["mp_valid"]), -2.0, np.float32))
    M.update_map_points_ref(dict(twc=ba["kf_twc"], valid=ref["kf_valid"], oct=ba["kf_oct"]),
                            dict(pos=m["mp_pos"], valid=ref["mp_valid"], ref_kf=ref["mp_ref_kf"], obs_ptr=ref["obs_ptr"], obs_kf=ref["obs_kf"], obs_feat=ref["obs_feat"]),
                            out, what=2)
    same(a["mp"], out, "refresh", list(out))


# ---- the pass

def test_mapping_pass_equals_the_host_edits(gpu, map_v1, gt_sync):
    """api.mapping_pass_from_map on the geometric scene (octaves clamped so that key-frames are culled) = joint_optimization_from_map
    followed by the restatement's erase / connections / cull / remove on the host: the map's arrays and the bookkeeping lists, bit for bit"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    m, ba, kf = S.geometric_scene(mean, cov, gt_sync["V1_01_easy"], cam)
    ba["kf_oct"] = np.minimum(ba["kf_oct"], 1).astype(np.int32)
    rng = np.random.default_rng(8)
    depth = rng.uniform(0.2, 8.0, ba["kf_oct"].shape).astype(np.float32)
    depth[ba["kf_uvr"][:, :, 2] < 0] = -1.0
    ref_kf = ES.first_entry_kf(m)
    g = api.GMM(ctx, mean, cov)
    caps = (24, 24, 2048, 16384)
    # the host route: the BA from the resident map, then the edits on the host's rows
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    r = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, caps)
    torch.cuda.synchronize()
    erased = r["erase_obs"].cpu().numpy()
    assert len(erased) > 0
    rows1, _ = E.map_remove(m, ba, erase_obs=erased, mp_ref_kf=ref_kf)
    m1, ba1 = E.apply_rows(m, ba, rows1)
    # the scene is small (the BA erases a tenth of its observations): so that key-frames ARE culled, only the points that still have five
    # observers after the erase keep a depth - an input of both routes, fixed before the device route runs
    depth[(m1["kf_mp"] < 0) | (np.diff(m1["obs_ptr"])[np.maximum(m1["kf_mp"], 0)] < 5)] = -1.0
    conn = R.connections_vec(m1, kf)
    cand = conn["conn_kf"][:64]
    cull = E.Model(m1, ba1).remove_key_frames(cand, depth, ES.TH_DEPTH)
    rows2, _ = E.map_remove(m1, ba1, rm_kf=cull["cull_rows"], mp_ref_kf=rows1["mp_ref_kf"])
    print("pass: erased", len(erased), "dead by erase", len(rows1["dead_mp"]), "candidates", len(cand), "culled", len(cull["cull_rows"]), "dead by cull",
          len(rows2["dead_mp"]), cull["num_mps"].tolist(), cull["num_redundant"].tolist())
    assert len(cull["cull_rows"]) >= 1 and len(rows2["dead_mp"]) >= 1
    # the device route
    md2, bd2 = to_dev(torch, m), to_dev(torch, ba)
    rk = torch.from_numpy(ref_kf.copy()).cuda()
    p = api.mapping_pass_from_map(ctx, g, cam, prm, md2, bd2, kf, caps, torch.from_numpy(depth).cuda(), ES.TH_DEPTH, mp_ref_kf=rk)
    torch.cuda.synchronize()
    assert p["erased"] == erased.tolist() and p["dead_by_erase"] == rows1["dead_mp"].tolist()
    assert p["culled"] == cull["cull_rows"].tolist() and p["dead_by_cull"] == rows2["dead_mp"].tolist() and p["status"] == (0, 0)
    n = len(rows2["obs_kf"])
    got = {k: md2[k].cpu().numpy() for k in MAP_KEYS}
    got.update(obs_kf=p["map"]["obs_kf"].cpu().numpy(), obs_feat=p["ba_rows"]["obs_feat"].cpu().numpy(), mp_ref_kf=rk.cpu().numpy())
    assert len(got["obs_kf"]) == n
    same(got, rows2, "pass", MAP_KEYS + ("obs_kf", "obs_feat", "mp_ref_kf"))
    for k in ("kf_pose", "kf_twc", "mp_assoc"):
        assert bd2[k].cpu().numpy().tobytes() == bd[k].cpu().numpy().tobytes(), k
    assert md2["mp_pos"].cpu().numpy().tobytes() == md["mp_pos"].cpu().numpy().tobytes()
    assert np.array_equal(p["cull"]["cull"][0, :len(cand)].cpu().numpy(), cull["cull"])


# ---- determinism, arguments

def test_twenty_runs_give_the_same_bytes(gpu):
    """integer stores and atomicMin only: the same call 20 times in one process, each on a fresh upload - a check of the design"""
    torch, ctx = gpu
    sc = ES.scene("small", True)
    rm_mp, erase, rm_kf = ES.dirty(sc, *ES.removals(sc, 3))
    Ccap = len(sc["cand"]) + 6
    cand, n_cand = lists_of(sc, Ccap)
    out = cull_out(len(cand), Ccap)
    md, bd = to_dev(torch, sc["m"]), to_dev(torch, sc["ba"])
    first = None
    for _ in range(20):
        c = device_cull(torch, ctx, md, bd, sc, cand, n_cand, out)
        d, _ = device_remove(torch, ctx, sc, rm_mp, erase, rm_kf)
        got = b"".join(c[k].tobytes() for k in CULL_KEYS) + b"".join(np.asarray(d[k]).tobytes() for k in ROW_KEYS + ("nobs", "status", "n_dead"))
        first = got if first is None else first
        assert got == first


def test_arguments(gpu):
    """B = 0 is a no-op; bad arguments are refused by the wrapper or by the library's own checks"""
    import ctypes as C
    torch, ctx = gpu
    sc = ES.scene("tiny")
    md, bd = to_dev(torch, sc["m"]), to_dev(torch, sc["ba"])
    depth = torch.from_numpy(sc["kf_depth"]).cuda()
    z = lambda *sh: torch.zeros(sh, dtype=torch.int32, device="cuda")
    api.cull_keyframes(ctx, md, bd, depth, 6.0, z(0, 8), z(0))
    for kw, msg in ((dict(depth=depth.double()), "float32"), (dict(depth=depth[:, :-1].contiguous()), "shape"), (dict(n=z(3)), "shape"),
                    (dict(bd={k: v for k, v in bd.items() if k != "kf_oct"}), "missing")):
        with pytest.raises(AssertionError, match=msg):
            api.cull_keyframes(ctx, md, kw.get("bd", bd), kw.get("depth", depth), 6.0, z(2, 8), kw.get("n", z(2)))
    with pytest.raises(AssertionError, match="both are needed"):
        api.map_remove(ctx, {k: v for k, v in md.items() if k != "kf_valid"}, bd, rm_kf=z(1))
    with pytest.raises(AssertionError, match="int32"):
        api.map_remove(ctx, md, bd, rm_kf=z(1).long())
    v, dev = api._map_view(md, False)
    w = api._map_ba_view(bd, v, dev)
    assert ctx.lib.gl_cull_keyframes(ctx.h, C.byref(v), C.byref(w), api._ptr(depth), 6.0, 1, 0, None, None, None, None, None, None, None, None) == -1
    assert ctx.lib.gl_last_error_string().decode().endswith("bad B / Ccap")
    assert ctx.lib.gl_map_remove(ctx.h, v.NMP, v.NKF, v.NFK, v.NOBS, None, None, 0, None, None) == -1
    assert ctx.lib.gl_last_error_string().decode().endswith("null argument")
