"""gl_update_connections, gl_ba_window_build and gl_ba_window_apply against tests/ba_window_ref.py - integers and copies, so equality
is exact and the entries behind every slab's contents must keep their sentinels - and the local BA from the resident map
(api.joint_optimization_from_map) against the same BA on the restatement's window uploaded by the host, bit for bit.  The scenes and
the conditions they meet: tests/ba_window_scenes.py, tests/test_ba_window_ref.py."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import map_point_ref as M
from tests.gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

SLAB_KEYS = R.WINDOW_ARRAYS + ("sizes", "status")


def to_host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def conn_out(B, Ccap, NKF=None):
    out = dict(conn_kf=np.full((B, Ccap), -7, np.int32), conn_w=np.full((B, Ccap), -7, np.int32), n_conn=np.full(B, -7, np.int32),
               status=np.full(B, -7, np.int32))
    if NKF is not None:
        out["kf_count"] = np.full((B, NKF), -7, np.int32)
    return out


def device_connections(torch, ctx, md, rows, out):
    od = to_dev(torch, out)
    api.update_connections(ctx, md, torch.from_numpy(np.asarray(rows, np.int32)).cuda(), out=od)
    torch.cuda.synchronize()
    return to_host(od)


def device_build(torch, ctx, md, bd, rows, slab):
    sd = to_dev(torch, slab)
    api.ba_window_build(ctx, md, bd, torch.from_numpy(np.asarray(rows, np.int32)).cuda(), sd)
    torch.cuda.synchronize()
    return to_host(sd)


def assert_same(dev, ref, what, keys=None):
    for k in (keys or ref):
        assert dev[k].dtype == ref[k].dtype and dev[k].tobytes() == ref[k].tobytes(), \
            (what, k, np.nonzero((dev[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[0][:8])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_update_connections_equals_the_restatement(gpu, name):
    """lists, weights, true counts, kf_count and status behind their sentinels, batched and one key-frame at a time; without kf_count;
    with a capacity below the list"""
    torch, ctx = gpu
    m, ba, rows = S.scene(name)
    md = to_dev(torch, m)
    B, NKF = len(rows), m["kf_mp"].shape[0]
    n = [len(R.connections_vec(m, int(kf))["conn_kf"]) for kf in rows]
    Ccap = max(n) + 4
    out = conn_out(B, Ccap, NKF)
    ref = R.update_connections(m, rows, out)
    assert_same(device_connections(torch, ctx, md, rows, out), ref, name)
    for b in range(min(B, 3)):
        one = {k: v[b:b + 1] for k, v in out.items()}
        assert_same(device_connections(torch, ctx, md, rows[b:b + 1], one), {k: v[b:b + 1] for k, v in ref.items()}, (name, b))
    lean = conn_out(B, Ccap)
    assert_same(device_connections(torch, ctx, md, rows, lean), R.update_connections(m, rows, lean), name + " without kf_count")
    if max(n) >= 2:
        short = conn_out(B, max(n) - 1, NKF)
        ref = R.update_connections(m, rows, short)
        assert (ref["status"] & R.CONN_TRUNCATED).any()
        assert_same(device_connections(torch, ctx, md, rows, short), ref, name + " truncated")


@pytest.mark.parametrize("name", list(S.SCENES))
def test_ba_window_build_equals_the_restatement(gpu, name):
    """every array of every slab, the true sizes, status and the back-maps; the entries behind the contents keep their sentinels (the
    guard of every slab: the next slab starts right behind); twice the same bytes"""
    torch, ctx = gpu
    m, ba, rows = S.scene(name)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    _, wins = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
    caps = S.caps_of(wins)
    slab = S.empty_slab(len(rows), caps)
    ref, _ = R.ba_window_build(m, ba, rows, slab)
    assert not (ref["status"] & R.TRUNCATED).any() and (ref["sizes"][:, 2] > 0).any()
    dev = device_build(torch, ctx, md, bd, rows, slab)
    assert_same(dev, ref, name, SLAB_KEYS)
    again = device_build(torch, ctx, md, bd, rows, slab)
    assert all(again[k].tobytes() == dev[k].tobytes() for k in SLAB_KEYS)


@pytest.mark.parametrize("which", range(4))
def test_ba_window_build_truncation(gpu, which):
    """each capacity in turn one below the largest window: the bit is set, sizes stay true, nothing is written behind a capacity"""
    torch, ctx = gpu
    m, ba, rows = S.scene("small")
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    _, wins = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
    caps = list(S.caps_of(wins, slack=0))
    caps[which] -= 1
    slab = S.empty_slab(len(rows), caps)
    ref, _ = R.ba_window_build(m, ba, rows, slab)
    assert (ref["status"] & (2 << which)).any() and not (ref["status"] & (R.TRUNCATED & ~(2 << which))).any()
    assert_same(device_build(torch, ctx, md, bd, rows, slab), ref, which, SLAB_KEYS)


@pytest.mark.parametrize("name", ["small", "kf_over_bound"])
def test_malformed_input_is_skipped(gpu, name):
    """rows outside the tables in kf_mp, obs_kf, obs_feat and kf_row, CSR ranges outside [0, NOBS] (words in LDS and in global memory):
    skipped as the restatement skips them, every output still exact behind its sentinels"""
    torch, ctx = gpu
    m, ba, rows = S.scene(name)
    S.malform(m, ba, 5)
    rows = rows.copy()
    rows[2], rows[3] = -1, m["kf_mp"].shape[0]
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    _, wins = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
    slab = S.empty_slab(len(rows), S.caps_of(wins))
    ref, _ = R.ba_window_build(m, ba, rows, slab)
    assert (ref["status"] == R.BAD_ROW).sum() == 2 and (ref["sizes"][:, 3] > 0).any()
    assert_same(device_build(torch, ctx, md, bd, rows, slab), ref, name, SLAB_KEYS)
    out = conn_out(len(rows), 64, m["kf_mp"].shape[0])
    assert_same(device_connections(torch, ctx, md, rows, out), R.update_connections(m, rows, out), name)


def test_ba_window_build_does_not_depend_on_the_batch(gpu):
    torch, ctx = gpu
    m, ba, rows = S.scene("small")
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    _, wins = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
    caps = S.caps_of(wins)
    assert len(rows) == 16
    batch = device_build(torch, ctx, md, bd, rows, S.empty_slab(16, caps))
    for b in (0, 1, 7, 15):
        one = device_build(torch, ctx, md, bd, rows[b:b + 1], S.empty_slab(1, caps))
        assert all(one[k][0].tobytes() == batch[k][b].tobytes() for k in SLAB_KEYS), b


def fake_ba_outputs(slab, rng):
    """slabs "after a BA" whose values depend on the map row alone (windows of a batch overlap: they then write the same bytes)"""
    B = slab["sizes"].shape[0]
    s = {k: v.copy() for k, v in slab.items()}
    for b in range(B):
        P, F, L, nobs = s["sizes"][b]
        kf, mp = s["win_kf"][b, :P].astype(np.float64), s["win_mp"][b, :L].astype(np.float64)
        s["poses"][b, :P] = np.stack([np.sin(kf * (c + 1)) + (2.0 if c == 3 else 0.0) for c in range(7)], 1)
        s["points"][b, :L] = np.stack([np.cos(mp * (c + 1)) * 3 for c in range(3)], 1)
    dropped = np.zeros(s["assoc"].shape, np.uint8)
    dropped[(np.maximum(s["win_mp"], 0) % 5 == 0)] = 1
    erase = (rng.uniform(size=s["obs_pose"].shape) < 0.03).astype(np.uint8)
    iters = rng.integers(1, 40, B).astype(np.int32)
    iters[B // 2] = 0  # the stop word was set on entry: nothing ran
    return s, dropped, erase, iters


@pytest.mark.parametrize("name", ["small", "clique"])
def test_ba_window_apply_equals_a_numpy_scatter(gpu, name):
    """the resident arrays after the write-back, whole arrays, bitwise: kf_pose, kf_twc by the stated expression, mp_pos, mp_assoc;
    erase_obs ascending = the mapped flags; a window whose iters is 0 applies nothing; then gl_update_map_points(what = 2) on the
    updated rows equals tests/map_point_ref.py"""
    torch, ctx = gpu
    m, ba, rows = S.scene(name)
    rng = np.random.default_rng(9)
    _, wins = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
    built, _ = R.ba_window_build(m, ba, rows, S.empty_slab(len(rows), S.caps_of(wins)))
    slab, dropped, erase, iters = fake_ba_outputs(built, rng)
    before = dict(kf_pose=ba["kf_pose"], kf_twc=ba["kf_twc"], mp_pos=m["mp_pos"], mp_assoc=ba["mp_assoc"])
    ref, lists = R.ba_window_apply(before, slab, dropped, erase, iters)
    assert any(len(l) > 1 for l in lists) and not np.array_equal(ref["mp_assoc"], before["mp_assoc"])
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    B, Ocap = erase.shape
    sd = to_dev(torch, dict(slab, dropped=dropped, erase=erase, iters=iters, erase_obs=np.full((B, Ocap), -7, np.int32), n_erase=np.full(B, -7, np.int32)))
    eo, ne = api.ba_window_apply(ctx, md, bd, sd)
    torch.cuda.synchronize()
    got = dict(kf_pose=bd["kf_pose"], kf_twc=bd["kf_twc"], mp_pos=md["mp_pos"], mp_assoc=bd["mp_assoc"])
    assert_same(to_host(got), ref, name)
    eo, ne = eo.cpu().numpy(), ne.cpu().numpy()
    for b in range(B):
        assert ne[b] == len(lists[b]) and np.array_equal(eo[b, :ne[b]], lists[b]) and (eo[b, ne[b]:] == -7).all(), b
        assert (np.diff(lists[b]) > 0).all()
    assert ne[B // 2] == 0
    # without kf_twc
    bd2 = to_dev(torch, {k: v for k, v in ba.items() if k != "kf_twc"})
    md2 = to_dev(torch, m)
    api.ba_window_apply(ctx, md2, bd2, sd)
    torch.cuda.synchronize()
    assert bd2["kf_pose"].cpu().numpy().tobytes() == ref["kf_pose"].tobytes() and md2["mp_pos"].cpu().numpy().tobytes() == ref["mp_pos"].tobytes()
    # the refresh the mapping thread runs next, on the rows as they now are
    NMP = len(m["mp_valid"])
    ref_kf = m["obs_kf"][np.minimum(m["obs_ptr"][:-1], len(m["obs_kf"]) - 1)].astype(np.int32)
    kf = dict(twc=ref["kf_twc"], valid=m["kf_valid"], oct=ba["kf_oct"])
    mp = dict(pos=ref["mp_pos"], valid=m["mp_valid"], ref_kf=ref_kf, obs_ptr=m["obs_ptr"], obs_kf=m["obs_kf"], obs_feat=ba["obs_feat"])
    out = dict(normal=np.full((NMP, 3), -7.0), max_dist=np.full(NMP, -1.0, np.float32), min_dist=np.full(NMP, -2.0, np.float32))
    od = to_dev(torch, out)
    api.update_map_points(ctx, dict(twc=bd["kf_twc"], valid=md["kf_valid"], oct=bd["kf_oct"]),
                          dict(pos=md["mp_pos"], valid=md["mp_valid"], ref_kf=torch.from_numpy(ref_kf).cuda(), obs_ptr=md["obs_ptr"], obs_kf=md["obs_kf"],
                               obs_feat=bd["obs_feat"]), od, what=2)
    torch.cuda.synchronize()
    M.update_map_points_ref(kf, mp, out, what=2)
    assert_same(to_host(od), out, name + " refresh")


@pytest.mark.parametrize("mode", [1, 2])  # the persistent kernel / the pipelined shape
def test_joint_optimization_from_map_equals_the_uploaded_window(gpu, oracle, map_v1, gt_sync, opt, mode):
    """end to end on the geometric scene: build -> sizes -> BA -> apply gives the same bits as api.joint_optimization on the
    restatement's window uploaded by the host - poses, points, dropped and erase flags, iters - and that run is within the tolerance
    tests/test_gpu_ba.py::check applies to the oracle; the resident rows end as the numpy scatter of those outputs.  The first
    capacities are too small: the slab is grown once."""
    from tests.test_gpu_ba import check
    torch, ctx = gpu
    opt("bagen_mode", mode)
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    m, ba, kf = S.geometric_scene(mean, cov, gt_sync["V1_01_easy"], cam)
    w = R.window_vec(m, ba, kf)
    P, F, L, nobs = w["P"], w["F"], w["L"], w["nobs"]
    g = api.GMM(ctx, mean, cov)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poses, points = T(w["poses"][None]), T(w["points"][None])
    dropped, erase, iters = api.joint_optimization(ctx, g, cam, prm, P, F, poses, T(w["prior"][None]), points, T(w["assoc"][None]),
                                                   T(w["obs_ptr"][None]), T(w["obs_pose"][None]), T(w["obs_uvr"][None]), T(w["obs_oct"][None]))
    torch.cuda.synchronize()
    up = [x.cpu().numpy() for x in (poses, points, dropped, erase, iters)]
    h = oracle.gmm_create(mean, cov)
    prob = dict(P=P, F=F, poses=w["poses"], prior=w["prior"], points=w["points"], obs_ptr=w["obs_ptr"], obs_pose=w["obs_pose"], obs_uvr=w["obs_uvr"],
                obs_oct=w["obs_oct"])
    check([prob], [w["assoc"]], up, oracle, h, cam)
    oracle.gmm_destroy(h)
    assert up[4][0] > 0 and not np.array_equal(up[0][0, :P], w["poses"][:P])
    for caps in ((4, 2, 100, 500), (P + 3, F + 3, L + 50, nobs + 100)):
        md, bd = to_dev(torch, m), to_dev(torch, ba)
        r = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, caps)
        torch.cuda.synchronize()
        assert (r["P"], r["F"], r["L"], r["nobs"]) == (P, F, L, nobs) and not r["status"] & R.TRUNCATED
        s = to_host(r["slab"])
        assert np.array_equal(s["win_kf"][0, :P + F], w["win_kf"]) and np.array_equal(s["win_mp"][0, :L], w["win_mp"])
        assert s["poses"][0, :P + F].tobytes() == up[0][0].tobytes() and s["points"][0, :L].tobytes() == up[1][0].tobytes()
        assert np.array_equal(s["dropped"][0, :L], up[2][0]) and np.array_equal(s["erase"][0, :nobs], up[3][0]) and s["iters"][0] == up[4][0]
        before = dict(kf_pose=ba["kf_pose"], kf_twc=ba["kf_twc"], mp_pos=m["mp_pos"], mp_assoc=ba["mp_assoc"])
        ref, lists = R.ba_window_apply(before, {k: s[k] for k in SLAB_KEYS}, s["dropped"], s["erase"], s["iters"])
        got = dict(kf_pose=bd["kf_pose"], kf_twc=bd["kf_twc"], mp_pos=md["mp_pos"], mp_assoc=bd["mp_assoc"])
        assert_same(to_host(got), ref, caps)
        assert np.array_equal(r["erase_obs"].cpu().numpy(), lists[0])
        assert np.array_equal(r["assoc_dropped"].cpu().numpy(), up[2][0]) and np.array_equal(r["win_kf"].cpu().numpy(), w["win_kf"])


def test_a_stop_word_set_on_entry_applies_nothing(gpu, map_v1, gt_sync):
    torch, ctx = gpu
    mean, cov = map_v1
    cam, prm = api.Camera(), api.Params()
    m, ba, kf = S.geometric_scene(mean, cov, gt_sync["V1_01_easy"], cam)
    g = api.GMM(ctx, mean, cov)
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    stop = torch.ones(1, dtype=torch.int32, device="cuda")
    r = api.joint_optimization_from_map(ctx, g, cam, prm, md, bd, kf, (24, 24, 1600, 8000), stop_flag=stop)
    torch.cuda.synchronize()
    assert int(r["iters"][0]) == 0 and len(r["erase_obs"]) == 0 and r["L"] > 300
    for k in ("kf_pose", "kf_twc", "mp_assoc"):
        assert bd[k].cpu().numpy().tobytes() == ba[k].tobytes(), k
    assert md["mp_pos"].cpu().numpy().tobytes() == m["mp_pos"].tobytes()


def test_arguments(gpu):
    """B = 0 is a no-op; bad arguments are refused by the wrapper or by the library's own checks"""
    import ctypes as C
    torch, ctx = gpu
    m, ba, rows = S.scene("tiny")
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    api.update_connections(ctx, md, none, Ccap=8)
    api.ba_window_build(ctx, md, bd, none, api.ba_window_slab(0, 4, 4, 16, 64))
    slab = api.ba_window_slab(2, 4, 4, 16, 64)
    rw = torch.from_numpy(rows[:2].copy()).cuda()
    for kw, msg in ((dict(bd=dict(bd, kf_oct=bd["kf_oct"].long())), "int32"), (dict(bd=dict(bd, kf_uvr=bd["kf_uvr"][:, :-1].contiguous())), "shape"),
                    (dict(bd={k: v for k, v in bd.items() if k != "mp_assoc"}), "missing"), (dict(slab=dict(slab, win_obs=slab["win_obs"][:, :-1].contiguous())), "shape"),
                    (dict(rows=rw[:1]), "shape")):
        with pytest.raises(AssertionError, match=msg):
            api.ba_window_build(ctx, md, kw.get("bd", bd), kw.get("rows", rw), kw.get("slab", slab))
    v, dev = api._map_view(md, False)
    w = api._map_ba_view(bd, v, dev)
    win, _ = api._ba_window(slab, dev)
    win.Lcap = 0
    assert ctx.lib.gl_ba_window_build(ctx.h, C.byref(v), C.byref(w), 2, api._ptr(rw), C.byref(win)) == -1
    assert ctx.lib.gl_last_error_string().decode().endswith("bad Pcap / Fcap / Lcap / Ocap")
    assert ctx.lib.gl_update_connections(ctx.h, C.byref(v), 2, api._ptr(rw), 0, None, None, None, None, None) == -1
    assert ctx.lib.gl_last_error_string().decode().endswith("bad B / Ccap")
