"""Every case of tests/map_cases.py on the device: gl_update_connections, gl_ba_window_build, gl_cull_keyframes, gl_map_remove,
gl_update_local_map and gl_update_map_points, each case alone (B = 1) and, where cases share a map, several rows in one batch with the
first of them twice.  Every output starts as sentinels and is compared byte for byte with the DECLARED arrays of the case - never with
anything the device made; what lies behind a list's contents must still be sentinels; after a reader the map's arrays are what they
were.  The structural cases (rank_selected with 1 023, 1 024 and 1 025 selected key-frames, the per-key-frame words in LDS and in
global memory) are held to connections_seq / window_seq.  That the declarations are what the restatements give: tests/test_map_cases.py."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import ba_window_ref as R
from tests import map_cases as MC
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.gpu_helpers import stop_on_device_error, to_dev  # noqa: F401  (autouse: the same after every test of this module)
from tests.test_gpu_ba_window import device_build, device_connections
from tests.test_gpu_local_map import device_update
from tests.test_gpu_map_edit import device_cull

pytestmark = pytest.mark.gpu


def same(got, want, what, keys=None):
    for k in (keys or want):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a.ravel()[:24], b.ravel()[:24])


def unchanged(dev, host, what):
    for k, v in host.items():
        if isinstance(v, np.ndarray):
            assert dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), (what, k, "a reader wrote to the map")


def stacked(arrays):
    """the B = 1 buffers of several cases as one batch"""
    return {k: np.concatenate([a[k] for a in arrays]) for k in arrays[0]}


def groups(table, key, shapes=True):
    """the cases of a table that one call can take together: the same map, the same arguments but `key` (of the same shape) -> lists of
    names, each with its first case once more at the end (the same row twice in a batch)"""
    by = {}
    for name, c in table.items():
        ins = c.inputs()
        sig = tuple((k, ins[k].shape, ins[k].tobytes()) for k in sorted(ins) if k not in key) + tuple((k, np.shape(c.args[k])) for k in key if shapes)
        by.setdefault(sig, []).append(name)
    return [g + g[:1] for g in by.values()]


def ids(gs):
    return ["+".join(g) for g in gs]


# ---- gl_update_connections

def conn_on_device(gpu, m, rows, out):
    torch, ctx = gpu
    md = to_dev(torch, m)
    got = run(lambda t, c: device_connections(t, c, md, rows, out), torch, ctx)
    unchanged(md, m, "connections")
    return got


@pytest.mark.parametrize("name", list(MC.CONN))
def test_connections_case_alone(gpu, name):
    c = MC.CONN[name]
    got = conn_on_device(gpu, c.m, [c.args["kf"]], MC.conn_out(c.args["Ccap"], c.m["kf_mp"].shape[0]))
    same(got, MC.conn_arrays(c), name)


CONN_GROUPS = groups(MC.CONN, ("kf",))


@pytest.mark.parametrize("names", CONN_GROUPS, ids=ids(CONN_GROUPS))
def test_connections_cases_of_one_map_in_one_call(gpu, names):
    cs = [MC.CONN[n] for n in names]
    out = stacked([MC.conn_out(c.args["Ccap"], c.m["kf_mp"].shape[0]) for c in cs])
    same(conn_on_device(gpu, cs[0].m, [c.args["kf"] for c in cs], out), stacked([MC.conn_arrays(c) for c in cs]), names)


def test_connections_groups_share_a_map():
    assert any(len(set(g)) > 1 for g in CONN_GROUPS) and all(len(g) >= 2 for g in CONN_GROUPS)


# ---- gl_ba_window_build

def window_on_device(gpu, m, ba, rows, slab):
    torch, ctx = gpu
    md, bd = to_dev(torch, m), to_dev(torch, ba)
    got = run(lambda t, c: device_build(t, c, md, bd, rows, slab), torch, ctx)
    unchanged(md, m, "window")
    unchanged(bd, ba, "window")
    return got


@pytest.mark.parametrize("name", list(MC.WINDOW))
def test_window_case_alone(gpu, name):
    c = MC.WINDOW[name]
    same(window_on_device(gpu, c.m, c.ba, [c.args["kf"]], MC.empty_slab(c.args["caps"])), MC.window_arrays(c), name)


WINDOW_GROUPS = groups(MC.WINDOW, ("kf",))


@pytest.mark.parametrize("names", WINDOW_GROUPS, ids=ids(WINDOW_GROUPS))
def test_window_cases_of_one_map_in_one_call(gpu, names):
    """every window twice (or with the others of its map) in one batch: each slab is the declared one, its neighbour's sentinels intact"""
    cs = [MC.WINDOW[n] for n in names]
    slab = stacked([MC.empty_slab(c.args["caps"]) for c in cs])
    same(window_on_device(gpu, cs[0].m, cs[0].ba, [c.args["kf"] for c in cs], slab), stacked([MC.window_arrays(c) for c in cs]), names)


# ---- gl_cull_keyframes

def cull_on_device(gpu, c, cand, n_cand, out):
    torch, ctx = gpu
    md, bd = to_dev(torch, c.m), to_dev(torch, c.ba)
    got = run(lambda t, x: device_cull(t, x, md, bd, c.args, cand, n_cand, out), torch, ctx)
    unchanged(md, c.m, "cull")
    unchanged(bd, c.ba, "cull")
    return got


@pytest.mark.parametrize("name", list(MC.CULL))
def test_cull_case_alone(gpu, name):
    c = MC.CULL[name]
    cand, n_cand, want = MC.cull_arrays(c)
    same(cull_on_device(gpu, c, cand, n_cand, MC.cull_out(cand.shape[1])), want, name)


CULL_GROUPS = groups(MC.CULL, ("cand",))


@pytest.mark.parametrize("names", CULL_GROUPS, ids=ids(CULL_GROUPS))
def test_cull_lists_of_one_map_in_one_call(gpu, names):
    """a workgroup per list, each with its own set of culled key-frames: `culled_earlier` and `culled_later` side by side"""
    cs = [MC.CULL[n] for n in names]
    parts = [MC.cull_arrays(c) for c in cs]
    cand, n_cand = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    out = stacked([MC.cull_out(cand.shape[1]) for _ in cs])
    same(cull_on_device(gpu, cs[0], cand, n_cand, out), stacked([p[2] for p in parts]), names)


def test_cull_groups_share_a_map():
    assert ["culled_earlier", "culled_later", "culled_earlier"] in CULL_GROUPS


# ---- gl_map_remove

def remove_on_device(torch, ctx, c):
    """gl_map_remove on a fresh upload -> (the rows of Model.to_rows + nobs, status, n_dead and what lies behind the new NOBS; the
    device dicts).  An empty list is not passed at all."""
    a = c.args
    md, bd = to_dev(torch, c.m), to_dev(torch, c.ba)
    rk = torch.from_numpy(a["mp_ref_kf"].copy()).cuda()
    kw = {k: torch.from_numpy(a[src].copy()).cuda() for k, src in (("rm_mp", "rm_mp"), ("erase_obs", "erase"), ("rm_kf", "rm_kf")) if len(a[src])}
    r = api.map_remove(ctx, md, bd, mp_ref_kf=rk, want_new_pos=True, **kw)
    torch.cuda.synchronize()
    n = r["nobs"]
    h = lambda t: t.cpu().numpy()
    rows = {k: h(md[k]) for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr")}
    rows.update(obs_kf=h(md["obs_kf"])[:n], obs_feat=h(bd["obs_feat"])[:n], mp_ref_kf=h(rk), obs_new_pos=h(r["obs_new_pos"]), dead_mp=h(r["dead_mp"]), nobs=n,
                status=r["status"], n_dead=r["n_dead"], tail_kf=h(md["obs_kf"])[n:], tail_feat=h(bd["obs_feat"])[n:])
    assert r["map"]["obs_kf"].shape[0] == n and r["ba"]["obs_feat"].shape[0] == n
    assert n == 0 or r["map"]["obs_kf"].data_ptr() == md["obs_kf"].data_ptr()  # (a view of the same buffer; an empty view has no address)
    return rows, (md, bd)


@pytest.mark.parametrize("name", list(MC.REMOVE))
def test_remove_case(gpu, name):
    torch, ctx = gpu
    c = MC.REMOVE[name]
    got, (md, bd) = run(lambda t, x: remove_on_device(t, x, c), torch, ctx)
    same(got, c.out, name, MC.ROW_KEYS)
    n = len(c.out["obs_kf"])
    assert got["nobs"] == n and got["status"] == c.out["status"] and got["n_dead"] == len(c.out["dead_mp"]), (name, got["nobs"], got["status"], got["n_dead"])
    assert np.array_equal(got["tail_kf"], c.m["obs_kf"][n:]) and np.array_equal(got["tail_feat"], c.ba["obs_feat"][n:]), (name, "written behind the new NOBS")
    for k in ("kf_uvr", "kf_oct", "kf_pose", "mp_assoc"):  # what the removal only reads
        assert bd[k].cpu().numpy().tobytes() == c.ba[k].tobytes(), (name, k)
    assert md["mp_pos"].cpu().numpy().tobytes() == c.m["mp_pos"].tobytes()


# ---- gl_update_local_map

def local_on_device(gpu, m, feat_mp, lists):
    torch, ctx = gpu
    md = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in m.items() if v is not None}
    fm, got = run(lambda t, c: device_update(t, c, m, feat_mp, lists, md), torch, ctx)
    unchanged(md, {k: v for k, v in m.items() if v is not None}, "local map")
    return fm, got


@pytest.mark.parametrize("name", list(MC.LOCAL))
def test_local_map_case_alone(gpu, name):
    c = MC.LOCAL[name]
    fm, got = local_on_device(gpu, c.m, np.array([c.args["feat_mp"]], np.int32), MC.local_lists(c))
    want_fm, want = MC.local_arrays(c)
    assert fm.dtype == want_fm.dtype and np.array_equal(fm, want_fm), (name, fm)
    same(got, want, name)


LOCAL_GROUPS = groups(MC.LOCAL, ("feat_mp",), shapes=False)


@pytest.mark.parametrize("names", LOCAL_GROUPS, ids=ids(LOCAL_GROUPS))
def test_local_map_frames_of_one_map_in_one_call(gpu, names):
    """the frames of one map as one batch, the shorter ones padded with features that hold nothing (-1: left as it is, counts nothing)"""
    cs = [MC.LOCAL[n] for n in names]
    NF = max(len(c.args["feat_mp"]) for c in cs)
    pad = lambda f: list(f) + [-1] * (NF - len(f))
    fm, got = local_on_device(gpu, cs[0].m, np.array([pad(c.args["feat_mp"]) for c in cs], np.int32), stacked([MC.local_lists(c) for c in cs]))
    assert np.array_equal(fm, np.array([pad(c.out["feat_mp"]) for c in cs], np.int32)), names
    same(got, stacked([MC.local_arrays(c)[1] for c in cs]), names)


def test_local_map_groups_share_a_map():
    assert any(len(set(g)) > 1 for g in LOCAL_GROUPS)


# ---- gl_update_map_points

def points_on_device(gpu, c):
    torch, ctx = gpu
    T = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    kd, pd, od = T(c.m), T(c.ba), T(MC.sentinel(len(c.ba["obs_ptr"]) - 1))

    def call(t, x):
        api.update_map_points(x, kd, pd, od, what=c.args["what"])
        t.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in od.items()}
    got = run(call, torch, ctx)
    unchanged(kd, c.m, "points")
    unchanged(pd, c.ba, "points")
    return got


@pytest.mark.parametrize("name", list(MC.POINTS))
def test_points_case(gpu, name):
    c = MC.POINTS[name]
    same(points_on_device(gpu, c), MC.points_arrays(c), name)


@pytest.mark.parametrize("name", list(MC.DESC_SETS))
def test_descriptor_set_alone(gpu, name):
    """one point in the launch: the packed path up to 32 observations, the whole wave on the point above"""
    c = MC.desc_case(name)
    same(points_on_device(gpu, c), MC.points_arrays(c), name)


def test_descriptor_sets_in_one_call(gpu):
    """all of them as the points of one map: the packed batches take several points at a time, the general path one after the other"""
    c = MC.desc_case(None)
    same(points_on_device(gpu, c), MC.points_arrays(c), "all")


# ---- rank_selected: the structural cases

@pytest.mark.parametrize("name", [n for n in MC.STRUCT if n.startswith("list")])
def test_covisible_list_of_about_1024_rows(gpu, name):
    """K = 1 023 / 1 024 (ranked in LDS) / 1 025 (counted over the whole table; words in LDS and in global memory): the list in full, cut
    at Ccap = K (status 0) and at K - 1 (the `r < Ccap` cut: the first K - 1 rows, the true length, the bit), and with kf 0 twice"""
    s = MC.struct_case(name)
    K, NKF = s["K"], s["m"]["kf_mp"].shape[0]
    seq = lambda m, kf: s["conn"]  # (connections_seq's lists, computed once)
    for Ccap, status in ((K + 3, 0), (K, 0), (K - 1, MC.TRUNCATED)):
        out = stacked([MC.conn_out(Ccap, NKF)] * 2)
        want = R.update_connections(s["m"], [0, 0], out, seq)
        assert want["status"].tolist() == [status] * 2 and want["n_conn"].tolist() == [K] * 2
        same(conn_on_device(gpu, s["m"], [0, 0], out), want, (name, Ccap))


@pytest.mark.parametrize("name", list(MC.STRUCT))
def test_window_with_about_1024_selected_key_frames(gpu, name):
    """`list_*`: K + 1 free poses, the covisible list ranked inside the build; `fixed_*`: P = 2 and 1 023 / 1 024 / 1 025 fixed key-frames
    in the order of their first observation, which is not the row order"""
    s = MC.struct_case(name)
    w = s["win"]
    caps = (w["P"] + 2, w["F"] + 2, w["L"] + 2, w["nobs"] + 5)
    slab = MC.empty_slab(caps)
    want, _ = R.ba_window_build(s["m"], s["ba"], [0], slab, lambda m, ba, kf: w)
    assert want["sizes"][0].tolist() == [w["P"], w["F"], w["L"], w["nobs"]] and want["status"][0] == 0
    same(window_on_device(gpu, s["m"], s["ba"], [0], slab), want, name)
