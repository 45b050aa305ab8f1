"""gl_tri_pair_setup and gl_create_map_points_from_map on the device:
  the pair set-up bit for bit against the numpy statement of its declared expression order, for the hand-built cases and for 64 seeded
    pose pairs under a camera with fx = fy and one with fx != fy; the skip bits exactly;
  every hand-built case of tests/create_points_cases.py: the declared outputs, integers exact, positions to 1e-9 against the sequential
    model with numpy_ref's functions; and bit for bit - integers and positions - against the SPLIT route on the device: the public
    gl_search_for_triangulation / gl_gather_triangulation_matches / gl_create_map_points fed the device's own fmat / epipole, the host
    carrying the mask in numpy and building the lists;
  a range split (n_nb = 1 + map_add, repeated) against one call with n_nb = nn + map_add: every resident array byte for byte;
  generated key-frames of NFK = 1, 63, 64, 65, 257 with nn = 1, 3, 10, 16 and 17 (an error, outputs untouched), k = 1, 5, 8, new_cap =
    NFK - 1 (an error);
  create_map_points_from_map against the split route followed by the host's map_add and refresh; a truncated map_add leaves the map's
    bytes untouched;
  the map's arrays are byte-identical before and after gl_create_map_points_from_map alone (every call of this file checks it)."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from oracle import numpy_ref
from tests import create_points_cases as cc
from tests import create_points_ref as ref
from tests import keyframe_cases as kc
from tests.gpu_helpers import T, gmm_of, stop_on_device_error  # noqa: F401 (the fixture is autouse)
from tests.test_create_points_ref import INT_KEYS, SEEDED_CAMS, check_ints, run_model, seeded_pairs

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
MAP_KEYS = ("kf_valid", "kf_mp", "mp_valid", "obs_ptr", "obs_kf")
BA_KEYS = ("kf_pose", "kf_twc", "kf_uvr", "kf_oct")
OUT_LISTS = ref.LIST_KEYS + ("new_pos",)


def dev_scene(torch, sc):
    """the scene's arrays on the device: (map view dict, ba dict, key-frame tables)"""
    return ({k: T(torch, sc.map[k]) for k in MAP_KEYS}, {k: T(torch, sc.ba[k]) for k in BA_KEYS}, {k: T(torch, v) for k, v in sc.kt.items()})


def dev_points(torch, ctx, sc, conn_kf, n_conn, first_nb, n_nb, mb, mp_base, dev=None, new_cap=None, prm=None):
    """gl_create_map_points_from_map alone -> the outputs on the host, the lists cut to n_new / n_attach; asserts that nothing is written
    behind the counts and that the inputs keep their bytes"""
    md, bd, kt = dev or dev_scene(torch, sc)
    cam = api.Camera(**sc.cam)
    g = gmm_of(ctx, sc.mean, sc.cov)
    before = {k: v.cpu().numpy().tobytes() for d in (md, bd, kt) for k, v in d.items()}
    out = map_grow.tri_points_out(sc.NFK, n_nb, new_cap=new_cap)
    for k in out:
        if k not in ("n_new", "n_attach", "status"):
            out[k].fill_(-77)
    o = map_grow.create_map_points_on_map(ctx, g, cam, prm or api.Params(), md, bd, kt, sc.kf_row, T(torch, np.asarray(conn_kf, np.int32)),
                                          T(torch, np.array([n_conn], np.int32)), first_nb=first_nb, n_nb=n_nb, mb=mb, mp_base=mp_base, out=out)
    torch.cuda.synchronize()
    after = {k: v.cpu().numpy().tobytes() for d in (md, bd, kt) for k, v in d.items()}
    assert before == after, "the map or a key-frame table was written"
    h = {k: v.cpu().numpy() for k, v in o.items()}
    n = int(h["n_new"][0])
    assert int(h["n_attach"][0]) == 2 * n
    r = {k: h[k][:n] for k in OUT_LISTS}
    r.update({k: h[k][:2 * n] for k in ref.ATT_KEYS})
    assert all((h[k][n:] == -77).all() for k in OUT_LISTS) and all((h[k][2 * n:] == -77).all() for k in ref.ATT_KEYS), "written behind n_new"
    r.update(n_new=n, n_attach=2 * n, feat_new=h["feat_new"], nb_stats=h["nb_stats"], skip=h["nb_stats"][:, 1].copy(), status=int(h["status"][0]), fmat=h["fmat"],
             epipole=h["epipole"])
    return r


def split_route(torch, ctx, sc, conn_kf, n_conn, first_nb, n_nb, mb, mp_base, o, prm=None, carry=True):
    """the route the call replaces, per neighbour on the device's own fmat / epipole: the public search (B = 1), gather and per-match
    block; the host carries the mask and builds the lists (the model's loop)"""
    cam = api.Camera(**sc.cam)
    g = gmm_of(ctx, sc.mean, sc.cov)
    ba, kt = sc.ba, sc.kt

    def side(row, has_mp):
        uvr = ba["kf_uvr"][row]
        d = dict(uv=uvr[:, :2], ur=uvr[:, 2].astype(f32), oct=ba["kf_oct"][row], angle=kt["angle"][row], desc=kt["desc"][row], has_mp=np.asarray(has_mp, np.uint8),
                 node_id=kt["node_id"][row], node_ptr=kt["node_ptr"][row], node_idx=kt["node_idx"][row], pose=ba["kf_pose"][row], depth=kt["depth"][row],
                 cand=kt["cand"][row], ncand=kt["ncand"][row])
        d = {k: T(torch, v[None]) for k, v in d.items()}
        d["nnode"] = T(torch, kt["nnode"][row:row + 1])
        return d

    state = {}

    def search(kf1, kf2, fmat, epipole):
        state["s1"], state["s2"] = side(kf1["row"], kf1["has_mp"]), side(kf2["row"], kf2["has_mp"])
        m, nm = api.search_for_triangulation(ctx, state["s1"], state["s2"], T(torch, fmat[None]), T(torch, epipole[None]), only_stereo=False, check_orientation=False)
        state["match"], state["nm"] = m, nm
        return m[0].cpu().numpy()

    def gather(kf2, match):
        off, m = api.gather_triangulation_matches(ctx, state["match"], state["nm"], state["s1"], state["s2"])
        n = int(off[1])
        a = {k: m[k][:n] for k in kc.CMP_KEYS}
        return a, m["idx1"][:n].cpu().numpy(), m["idx2"][:n].cpu().numpy()

    def create(**a):
        x, t, c = api.create_map_points(ctx, g, cam, prm or api.Params(), *[a[k] for k in kc.CMP_KEYS])
        return x.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()

    pairs = None if o is None else (o["skip"], o["nb_stats"][:, 0], o["fmat"], o["epipole"])  # (None: the numpy statement's, the same bits)
    return ref.create_points(sc.cam, sc.map, ba, kt, sc.kf_row, conn_kf, n_conn, first_nb, n_nb, mb, mp_base, search, create, pairs=pairs, gather=gather, carry=carry)


def same_bits(o, s, what):
    for k in INT_KEYS + ("new_pos",):
        a, b = np.asarray(o[k]), np.asarray(s[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a, b)


# ---- gl_tri_pair_setup ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_pair_setup_cases(gpu, name):
    torch, ctx = gpu
    c = cc.CASES[name]
    skip, fmat, epi = map_grow.tri_pair_setup(ctx, api.Camera(**c.cam), {k: T(torch, c.ba[k]) for k in ("kf_pose", "kf_twc")}, T(torch, c.map["kf_valid"]), c.kf_row,
                                              T(torch, c.conn_kf), T(torch, np.array([c.n_conn], np.int32)), first_nb=c.first_nb, n_nb=c.nn, mb=c.mb)
    torch.cuda.synchronize()
    ws, _, wf, we = ref.pair_setup(c.cam, c.map["kf_valid"], c.ba["kf_pose"], c.ba["kf_twc"], c.kf_row, c.conn_kf, c.n_conn, c.first_nb, c.nn, c.mb)
    assert np.array_equal(skip.cpu().numpy(), c.want["skip"]) and np.array_equal(ws, c.want["skip"])
    assert fmat.cpu().numpy().tobytes() == wf.tobytes(), (fmat.cpu().numpy(), wf)
    assert epi.cpu().numpy().tobytes() == we.tobytes(), (epi.cpu().numpy(), we)


@pytest.mark.parametrize("ci", [0, 1])
def test_pair_setup_seeded_pose_pairs(gpu, ci):
    """64 seeded pose pairs (Haar rotations, translations in [-2, 2]^3): key-frame 2 i + 1 is the neighbour of key-frame 2 i; ci = 1: a camera
    with fx != fy.  mb = 0: no baseline is short."""
    torch, ctx = gpu
    cam = SEEDED_CAMS[ci]
    pairs = seeded_pairs()
    pose = np.array([p for pr in pairs for p in pr])
    twc = np.array([-(ref_R(p).T @ p[4:]) for p in pose])
    ba = dict(kf_pose=T(torch, pose), kf_twc=T(torch, twc))
    one = T(torch, np.array([1], np.int32))
    got_f, got_e = [], []
    for i in range(len(pairs)):
        skip, fmat, epi = map_grow.tri_pair_setup(ctx, api.Camera(**cam), ba, None, 2 * i, T(torch, np.array([2 * i + 1], np.int32)), one, n_nb=1, mb=0.0)
        got_f.append(fmat)
        got_e.append(epi)
        assert int(skip[0]) == 0
    torch.cuda.synchronize()
    for i, (p1, p2) in enumerate(pairs):
        F, e = ref.fundamental_and_epipole(p1, p2, cam)
        assert got_f[i].cpu().numpy()[0].tobytes() == F.tobytes(), (i, got_f[i].cpu().numpy()[0], F)
        assert got_e[i].cpu().numpy()[0].tobytes() == e.tobytes(), (i, got_e[i].cpu().numpy()[0], e)


def ref_R(p):
    return np.array(ref._qtoR([float(v) for v in p[:4]]))


# ---- the hand-built cases -------------------------------------------------------------------------------------------------------------------
_model = {}


def model_of(name):
    """the model's outputs of a case with numpy_ref's functions: computed once, shared, never written to"""
    if name not in _model:
        _model[name] = run_model(cc.CASES[name], numpy_ref)
        for v in _model[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _model[name]


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case(gpu, name):
    torch, ctx = gpu
    c = cc.CASES[name]
    o = dev_points(torch, ctx, c, c.conn_kf, c.n_conn, c.first_nb, c.nn, c.mb, cc.MP_BASE)
    check_ints(o, c.want, name)
    m = model_of(name)
    print(name, "n_new", o["n_new"], "positions: max difference from the model", float(np.abs(o["new_pos"] - m["new_pos"]).max(initial=0.0)))
    assert o["new_pos"].shape == m["new_pos"].shape and np.allclose(o["new_pos"], m["new_pos"], rtol=0, atol=1e-9)
    assert o["fmat"].tobytes() == m["fmat"].tobytes() and o["epipole"].tobytes() == m["epipole"].tobytes()
    s = split_route(torch, ctx, c, c.conn_kf, c.n_conn, c.first_nb, c.nn, c.mb, cc.MP_BASE, o)
    same_bits(o, s, name)


# ---- generated key-frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NFK,nn,k", [(1, 1, 5), (63, 3, 5), (64, 10, 1), (65, 16, 8), (257, 10, 5), (257, 3, 8)])
def test_generated_equals_the_split_route(gpu, NFK, nn, k):
    torch, ctx = gpu
    sc = cc.generated(NFK, nn + 2, 100 + NFK + nn, k)
    conn = np.arange(1, nn + 2, dtype=np.int32)  # one more than nn: only the first nn
    mb = map_grow.default_mb(api.Camera(**sc.cam))
    o = dev_points(torch, ctx, sc, conn, len(conn), 0, nn, mb, sc.NMP)
    s = split_route(torch, ctx, sc, conn, len(conn), 0, nn, mb, sc.NMP, o)
    print("NFK", NFK, "nn", nn, "k", k, "nb_stats", o["nb_stats"][:, :5].tolist(), "types", np.bincount(o["new_type"], minlength=5).tolist())
    same_bits(o, s, (NFK, nn, k))
    if NFK >= 63:
        assert o["n_new"] > 0 and o["nb_stats"][0, 2] > 0  # (a later neighbour may find every shared feature taken)
    if NFK == 257 and nn == 10:
        nocarry = split_route(torch, ctx, sc, conn, len(conn), 0, nn, mb, sc.NMP, o, carry=False)  # (the B-pair batch's answer)
        assert nocarry["n_new"] != o["n_new"] or nocarry["new_feat1"].tobytes() != o["new_feat1"].tobytes(), "the carry decides nothing on this key-frame"


def test_argument_errors_leave_the_outputs_untouched(gpu):
    torch, ctx = gpu
    sc = cc.generated(64, 19, 7)
    dev = dev_scene(torch, sc)
    cam, g = api.Camera(**sc.cam), gmm_of(ctx, sc.mean, sc.cov)
    conn, n_conn = T(torch, np.arange(1, 19, dtype=np.int32)), T(torch, np.array([18], np.int32))
    for n_nb, new_cap in ((17, 64), (3, 63)):
        out = map_grow.tri_points_out(64, n_nb, new_cap=new_cap)
        for v in out.values():
            v.fill_(-77)
        with pytest.raises(api.GLError):
            map_grow.create_map_points_on_map(ctx, g, cam, api.Params(), *dev, 0, conn, n_conn, n_nb=n_nb, mb=0.1, mp_base=sc.NMP, out=out)
        torch.cuda.synchronize()
        assert all((v.cpu().numpy() == -77).all() for v in out.values()), "an argument error wrote an output"
    with pytest.raises(api.GLError):
        map_grow.tri_pair_setup(ctx, cam, dev[1], dev[0]["kf_valid"], 0, conn, n_conn, n_nb=17, mb=0.1)
    # nn = 16 runs
    o = dev_points(torch, ctx, sc, np.arange(1, 19, dtype=np.int32), 18, 0, 16, 0.1, sc.NMP, dev=dev)
    assert (o["skip"] == 0).sum() > 0


# ---- on the resident map: map_add behind the call ---------------------------------------------------------------------------------------------
def resident(torch, sc, extra_mp, extra_obs):
    from tests.test_gpu_map_grow import upload, with_point_arrays
    NMP = len(sc.map["mp_valid"])
    m = with_point_arrays({k: sc.map[k] for k in MAP_KEYS + ("mp_pos",)}, NMP + extra_mp)
    m["mp_pos"] = np.concatenate([sc.map["mp_pos"], np.full((extra_mp, 3), -7.0)])
    ba = {k: sc.ba[k] for k in BA_KEYS + ("obs_feat", "mp_assoc")}
    md, bd, rk, sizes = upload(torch, m, ba, sc.mp_ref_kf, NMP + extra_mp, len(sc.map["obs_kf"]) + extra_obs)
    return md, bd, rk, sizes


def snapshot(torch, md, bd, rk):
    torch.cuda.synchronize()
    return dict({"map." + k: v.cpu().numpy() for k, v in md.items() if hasattr(v, "cpu")}, **{"ba." + k: v.cpu().numpy() for k, v in bd.items() if hasattr(v, "cpu")},
                mp_ref_kf=rk.cpu().numpy())


def add_lists(torch, ctx, md, bd, rk, sizes, s):
    t = lambda a, dt=np.int32: T(torch, np.asarray(a, dt))
    return map_grow.map_add(ctx, md, bd, sizes, new_mp=dict(pos=t(s["new_pos"], f64).reshape(-1, 3), assoc=t(s["new_assoc"]), ref_kf=t(s["new_ref_kf"])),
                            attach=dict(mp=t(s["att_mp"]), kf=t(s["att_kf"]), feat=t(s["att_feat"])), mp_ref_kf=rk)


def on_resident(torch, ctx, sc, md, bd, kt, sizes, conn, first_nb, n_nb, mb):
    """gl_create_map_points_from_map on the capacity buffers cut to sizes -> the device's output dict"""
    m1, b1 = map_grow.map_views(md, bd, sizes)
    return map_grow.create_map_points_on_map(ctx, gmm_of(ctx, sc.mean, sc.cov), api.Camera(**sc.cam), api.Params(), {k: m1[k] for k in MAP_KEYS},
                                             {k: b1[k] for k in BA_KEYS}, kt, sc.kf_row, T(torch, conn), T(torch, np.array([len(conn)], np.int32)),
                                             first_nb=first_nb, n_nb=n_nb, mb=mb, mp_base=sizes[0])


@pytest.mark.parametrize("which", ["carry_created_feature_is_no_query", "rejected_match_asks_again", "generated"])
def test_range_split_equals_the_whole(gpu, which):
    torch, ctx = gpu
    if which == "generated":
        sc, nn = cc.generated(65, 6, 41), 4
        conn, mb = np.arange(1, 5, dtype=np.int32), map_grow.default_mb(api.Camera(**sc.cam))
    else:
        sc = cc.CASES[which]
        nn, conn, mb = sc.nn, sc.conn_kf, sc.mb
    kt = {k: T(torch, v) for k, v in sc.kt.items()}
    res = []
    for split in (False, True):
        md, bd, rk, sizes = resident(torch, sc, 2 * sc.NFK, 4 * sc.NFK)
        total = 0
        for first, n in ([(j, 1) for j in range(nn)] if split else [(0, nn)]):
            s = on_resident(torch, ctx, sc, md, bd, kt, sizes, conn, first, n, mb)
            r = map_grow.map_add(ctx, md, bd, sizes, new_mp=dict(pos=s["new_pos"], assoc=s["new_assoc"], ref_kf=s["new_ref_kf"]),
                                 attach=dict(mp=s["att_mp"], kf=s["att_kf"], feat=s["att_feat"]), mp_ref_kf=rk, n_new_mp=s["n_new"], n_attach=s["n_attach"])
            assert r["status"] == 0
            total += r["sizes"][0] - sizes[0]
            sizes = r["sizes"]
        res.append((sizes, total, snapshot(torch, md, bd, rk)))
    print(which, "new points", res[0][1], "sizes", res[0][0])
    assert res[0][1] > 0 and res[0][:2] == res[1][:2]
    for k in res[0][2]:
        assert res[0][2][k].tobytes() == res[1][2][k].tobytes(), k


def test_from_map_equals_the_split_route(gpu):
    """create_map_points_from_map (update_connections, the loop, map_add, the refresh) against the split route followed by the host's
    map_add and refresh: every resident array"""
    from tests.test_gpu_map_grow import refresh
    torch, ctx = gpu
    sc, nn = cc.generated(257, 6, 23), 4
    cam, g = api.Camera(**sc.cam), gmm_of(ctx, sc.mean, sc.cov)
    ktd = {k: T(torch, v) for k, v in sc.kt.items()}
    # the neighbours as gl_update_connections orders them (a covisibility weight per key-frame, ties to the lowest row)
    md, bd, rk, sizes = resident(torch, sc, 600, 1200)
    refresh(ctx, md, bd, rk, ktd["desc"], sizes)
    m1, _ = map_grow.map_views(md, bd, sizes)
    cn = api.update_connections(ctx, {k: m1[k] for k in MAP_KEYS}, T(torch, np.array([0], np.int32)), Ccap=nn)
    torch.cuda.synchronize()
    conn, n_conn = cn["conn_kf"][0].cpu().numpy(), int(cn["n_conn"][0])
    assert n_conn >= nn, "the generated key-frames share too few points to be covisible"
    mb = map_grow.default_mb(cam)
    o = dev_points(torch, ctx, sc, conn, n_conn, 0, nn, mb, sc.NMP)
    s = split_route(torch, ctx, sc, conn, n_conn, 0, nn, mb, sc.NMP, o)
    r0 = add_lists(torch, ctx, md, bd, rk, sizes, s)
    assert r0["status"] == 0
    refresh(ctx, md, bd, rk, ktd["desc"], r0["sizes"])
    host = snapshot(torch, md, bd, rk)
    md, bd, rk, sizes = resident(torch, sc, 600, 1200)
    refresh(ctx, md, bd, rk, ktd["desc"], sizes)
    r = map_grow.create_map_points_from_map(ctx, g, cam, api.Params(), md, bd, ktd, 0, nn=nn, sizes=sizes, mp_ref_kf=rk)
    assert r["status"] == 0 and r["sizes"] == r0["sizes"] and r["n_new"] == s["n_new"] > 10
    assert np.array_equal(r["new_type"].cpu().numpy(), s["new_type"]) and np.array_equal(r["feat_new"].cpu().numpy(), s["feat_new"])
    assert np.array_equal(r["nb_stats"].cpu().numpy(), s["nb_stats"])
    dev = snapshot(torch, md, bd, rk)
    print("new points", r["n_new"], "sizes", r["sizes"], "nb_stats", s["nb_stats"][:, :5].tolist())
    for k in host:
        assert host[k].tobytes() == dev[k].tobytes(), k


def test_from_map_after_a_truncation_changes_nothing(gpu):
    from tests.test_gpu_map_grow import refresh
    torch, ctx = gpu
    sc = cc.generated(257, 6, 23)
    cam, g = api.Camera(**sc.cam), gmm_of(ctx, sc.mean, sc.cov)
    ktd = {k: T(torch, v) for k, v in sc.kt.items()}
    for caps, bit in (((3, 1200), map_grow.GROW_MP_TRUNCATED), ((600, 3), map_grow.GROW_OBS_TRUNCATED)):
        md, bd, rk, sizes = resident(torch, sc, *caps)
        refresh(ctx, md, bd, rk, ktd["desc"], sizes)
        before = snapshot(torch, md, bd, rk)
        r = map_grow.create_map_points_from_map(ctx, g, cam, api.Params(), md, bd, ktd, 0, nn=4, sizes=sizes, mp_ref_kf=rk)
        assert r["status"] & bit and r["sizes"] == sizes and r["n_new"] > 3
        after = snapshot(torch, md, bd, rk)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), (k, bit)
