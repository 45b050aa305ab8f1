"""gl_create_stereo_points / gl_create_temporal_points on the device against the sequential model (tests/key_frame_create_ref.py):
  every hand-built case of tests/key_frame_create_cases.py: the declared outputs, integers exact, positions and pts0 to 1e-9 against the
    model with numpy_ref's check; and bit for bit - integers and positions - against the SPLIT route on the device's own pts0: the public
    gl_check_map_association with the host masking the octaves and walking;
  generated key-frames of NF = 1, 63, 64, 65, 101, 102, 1 024, 1 025 and GL_STEREO_WALK_MAX slots, and one above it (an error, outputs
    untouched); candidate tables of k = 1, 5, 8; B = 3 with the cases of one map concatenated in both orders, the same bits as alone;
  a seeded random key-frame of 1 200 features on map_v1 held to the model run on the device's own per-feature check results;
  process_key_frame_from_map against the split route on the host: every resident array after map_add and the refresh; a truncated
    map_add leaves the map's bytes untouched;
  the arrays gl_create_temporal_points writes, fed to gl_track_frame_chain, give the bits of the arrays the host makes."""
import numpy as np
import pytest

from gmmloc_amd import api, map_grow, synth
from oracle import numpy_ref
from tests import key_frame_create_cases as cc
from tests import key_frame_create_ref as ref
from tests import keyframe_cases as kc
from tests.gpu_helpers import T, gmm_of, stop_on_device_error  # noqa: F401 (the fixture is autouse)
from tests.test_key_frame_create_ref import INT_KEYS, check_stereo, check_temporal

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LISTS = ("new_feat", "new_assoc", "new_ref_kf", "att_mp", "att_kf", "att_feat")
IN_KEYS = tuple(api.STEREO_IN_DTYPES)


def padded(fr, NF, off=0):
    """the key-frame in NF slots from slot `off` on; the others are padding slots (octave -1) WITH a positive depth"""
    n = len(fr["feat_depth"])
    assert off + n <= NF
    out = {"pose": fr["pose"]}
    fill = dict(feat_uv=7.0, feat_ur=-1.0, feat_depth=1.0, feat_oct=-1, cand=-1, ncand=0, held=0, last_outlier=0, feat_desc=0)
    for k, v in fill.items():
        a = np.full((NF,) + fr[k].shape[1:], v, fr[k].dtype)
        a[off:off + n] = fr[k]
        out[k] = a
    return out


def recut(fr, k):
    """the candidate table in k columns (the lists must fit)"""
    assert fr["ncand"].max(initial=0) <= k
    c = -np.ones((len(fr["ncand"]), k), np.int32)
    w = min(k, fr["cand"].shape[1])
    c[:, :w] = fr["cand"][:, :w]
    return dict(fr, cand=c)


def stacked(torch, frames, rows):
    a = {k: T(torch, np.stack([f[k] for f in frames])) for k in IN_KEYS if k != "kf_row"}
    a["kf_row"] = T(torch, np.array(rows, np.int32))
    return a


def dev_stereo(torch, ctx, gmm, cam, frames, rows, mp_base, check_depth, th, prm=None):
    """B key-frames of one shape in one call -> per key-frame the outputs, the lists cut to n_new (and whole under 'raw')"""
    r = api.create_stereo_points(ctx, gmm, api.Camera(**cam), prm or api.Params(), stacked(torch, frames, rows), mp_base, check_depth, float(th), want_pts0=True)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in r.items()}
    outs = []
    for b in range(len(frames)):
        n = int(h["n_new"][b])
        o = {k: h[k][b][:n] for k in LISTS + ("new_pos",)}
        o.update(n_new=n, feat_new=h["feat_new"][b], stats=h["stats"][b], pts0=h["pts0"][b], raw={k: h[k][b] for k in LISTS + ("new_pos",)})
        assert all((o["raw"][k][n:] == 0).all() for k in o["raw"]), "written behind n_new"
        outs.append(o)
    return outs


def split_route(torch, ctx, gmm, cam, frames, pts0, rows, mp_base, check_depth, th, prm=None):
    """the route the call replaces, on the device's own pts0: the host masks the octaves (an entry, create_new, candidates), the public
    gl_check_map_association answers, the host walks (the model on those answers) -> per key-frame the model's outputs"""
    depth, octv = np.stack([f["feat_depth"] for f in frames]), np.stack([f["feat_oct"] for f in frames])
    held, ncand = np.stack([f["held"] for f in frames]), np.stack([f["ncand"] for f in frames])
    run = (depth > 0) & (octv >= 0) & (octv <= 7) & (held != 1) & (ncand > 0)
    uvr = np.concatenate([np.stack([f["feat_uv"] for f in frames]), np.stack([f["feat_ur"] for f in frames]).astype(f64)[..., None]], 2)
    pts = T(torch, np.stack(pts0))
    comp = api.check_map_association(ctx, gmm, api.Camera(**cam), prm or api.Params(), T(torch, np.stack([f["pose"] for f in frames])), pts, T(torch, uvr),
                                     T(torch, np.where(run, octv, -1).astype(np.int32)), T(torch, np.stack([f["cand"] for f in frames])), T(torch, ncand))
    torch.cuda.synchronize()
    comp, pts = comp.cpu().numpy(), pts.cpu().numpy()
    return [ref.stereo_walk(cam, f, ref.check_table(comp[b], pts[b]), mp_base, check_depth, th, rows[b], pts0=pts0[b]) for b, f in enumerate(frames)], comp


def same_bits(o, m, what):
    for k in INT_KEYS + ("new_pos", "pts0"):
        a, b = np.asarray(o[k]), np.asarray(m[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a, b)


def shifted(c, off, NF):
    """the declared outputs of a case that sits at slot `off` of NF"""
    w = dict(c.want)
    for k in ("new_feat", "att_feat"):
        w[k] = w[k] + off
    fn = -np.ones(NF, np.int32)
    fn[off:off + c.NF] = c.want["feat_new"]  # (the row of a new point counts the created points, not the slots)
    w["feat_new"] = fn
    return w


# ---- the hand-built cases ---------------------------------------------------------------------------------------------------------------
_model = {}


def model_of(name):
    """the model's outputs of a case with numpy_ref's check: computed once, shared, never written to"""
    if name not in _model:
        c = cc.CASES[name]
        with kc.Ref(numpy_ref, c.mean, c.cov) as r:
            _model[name] = ref.stereo_walk(c.cam, c.fr, ref.check_with(r, c.cam, c.fr), cc.MP_BASE, c.check_depth, c.th, cc.KF_ROW)
        for v in _model[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _model[name]


@pytest.mark.parametrize("name", cc.STEREO)
def test_stereo_case(gpu, name):
    torch, ctx = gpu
    c = cc.CASES[name]
    g = gmm_of(ctx, c.mean, c.cov)
    o = dev_stereo(torch, ctx, g, c.cam, [c.fr], [cc.KF_ROW], cc.MP_BASE, c.check_depth, c.th)[0]
    check_stereo(c, o)
    m = model_of(name)
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(o[k]), np.asarray(m[k])), (name, k)
    d = np.abs(o["new_pos"] - m["new_pos"])
    print(name, "new_pos: max difference to the model", float(np.nanmax(d)) if d.size else 0.0)
    assert np.allclose(o["new_pos"], m["new_pos"], rtol=0, atol=1e-9, equal_nan=True) and np.allclose(o["pts0"], m["pts0"], rtol=0, atol=1e-9, equal_nan=True)
    s, _ = split_route(torch, ctx, g, c.cam, [c.fr], [o["pts0"]], [cc.KF_ROW], cc.MP_BASE, c.check_depth, c.th)
    same_bits(o, s[0], (name, "split route"))


@pytest.mark.parametrize("k", [1, 5, 8])
def test_candidate_tables_of_k_columns(gpu, k):
    torch, ctx = gpu
    names = [n for n in cc.STEREO if cc.CASES[n].fr["ncand"].max() <= k]
    assert len(names) >= len(cc.STEREO) - (2 if k == 1 else 0)
    for n in names:
        c = cc.CASES[n]
        fr = recut(c.fr, k)
        o = dev_stereo(torch, ctx, gmm_of(ctx, c.mean, c.cov), c.cam, [fr], [cc.KF_ROW], cc.MP_BASE, c.check_depth, c.th)[0]
        check_stereo(c, o)
        same_bits(o, split_route(torch, ctx, gmm_of(ctx, c.mean, c.cov), c.cam, [fr], [o["pts0"]], [cc.KF_ROW], cc.MP_BASE, c.check_depth, c.th)[0][0], (n, k))


def _groups():
    g = {}
    for n in cc.STEREO:
        c = cc.CASES[n]
        g.setdefault((c.mean.tobytes(), c.cov.tobytes(), c.k, c.check_depth), []).append(n)
    return [v for v in g.values()]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_three_key_frames_in_one_call(gpu, order):
    """B = 3: the cases of one map (and one check_depth) three at a time, each at another slot of the common shape, with key-frame rows and
    an mp_base of their own call: the declared outputs, and the bits of the case alone"""
    torch, ctx = gpu
    seen = 0
    for names in _groups():
        names = names[::-1] if order == "reversed" else names
        while len(names) % 3:
            names = names + [names[0]]
        for i in range(0, len(names), 3):
            trio = [cc.CASES[n] for n in names[i:i + 3]]
            NF = max(c.NF for c in trio) + 5
            offs = [0, (NF - trio[1].NF) // 2, NF - trio[2].NF]
            frames = [padded(c.fr, NF, off) for c, off in zip(trio, offs)]
            g = gmm_of(ctx, trio[0].mean, trio[0].cov)
            outs = dev_stereo(torch, ctx, g, trio[0].cam, frames, [cc.KF_ROW] * 3, cc.MP_BASE, trio[0].check_depth, trio[0].th)
            for c, off, o in zip(trio, offs, outs):
                alone = dev_stereo(torch, ctx, g, c.cam, [c.fr], [cc.KF_ROW], cc.MP_BASE, c.check_depth, c.th)[0]
                w = shifted(c, off, NF)
                for k in INT_KEYS:
                    assert np.array_equal(np.asarray(o[k]), np.asarray(w[k])), (c.name, k, "declared", off)
                assert o["new_pos"].tobytes() == alone["new_pos"].tobytes() and o["pts0"][off:off + c.NF].tobytes() == alone["pts0"].tobytes(), c.name
                assert not o["pts0"][:off].any() and not o["pts0"][off + c.NF:].any(), (c.name, "pts0 of a padding slot")
                seen += 1
    assert seen >= len(cc.STEREO)


def test_rows_and_base_of_each_key_frame(gpu):
    """kf_row per key-frame and mp_base reach new_ref_kf / att_kf / att_mp"""
    torch, ctx = gpu
    c = cc.CASES["order_across_and_inside"]
    outs = dev_stereo(torch, ctx, gmm_of(ctx, c.mean, c.cov), c.cam, [c.fr, c.fr], [3, 11], 123456, 1, c.th)
    for o, row in zip(outs, (3, 11)):
        assert (o["new_ref_kf"] == row).all() and (o["att_kf"] == row).all() and np.array_equal(o["att_mp"], 123456 + np.arange(4))


# ---- generated key-frames: the shapes -----------------------------------------------------------------------------------------------------
def generated(NF):
    """depths 0.25 .. 6.25 in steps of 1 / 16 with many ties, scattered over the slots; slots without depth and padding slots; every held
    state; on MAP_MOVE no list, [0], [1] and [0, 1]"""
    i = np.arange(NF)
    feats = [cc.feat(-1.0 if j % 11 == 0 else 0.25 + ((j * 61) % 97) / 16.0, held=(j * 5 + 1) % 3, cand=((), (0,), (1,), (0, 1))[(j // 3) % 4], oct=-1 if j % 13 == 5 else j % 8)
             for j in i]
    return cc.frame(feats)


NFS = (1, 63, 64, 65, 101, 102, 1024, 1025, api.STEREO_WALK_MAX)


@pytest.mark.parametrize("check_depth", [0, 1])
@pytest.mark.parametrize("NF", NFS)
def test_shapes(gpu, NF, check_depth):
    torch, ctx = gpu
    mean, cov = kc.mk_map(cc.MAP_MOVE)
    g = gmm_of(ctx, mean, cov)
    fr = generated(NF)
    o = dev_stereo(torch, ctx, g, kc.CAM5, [fr], [2], 50, check_depth, cc.TH)[0]
    s, comp = split_route(torch, ctx, g, kc.CAM5, [fr], [o["pts0"]], [2], 50, check_depth, cc.TH)
    same_bits(o, s[0], ("generated", NF))
    st = o["stats"]
    print("NF", NF, "stats", st.tolist())
    if NF >= 1024:  # the key-frame exercises what it is for: rejected and accepted entries, and the break exactly when it is armed
        assert st[3] > 0 and st[4] > 100 and st[5] == check_depth and (st[1] < st[0]) == bool(check_depth)
    # the temporal walk on the same slots
    last = cc.last_rows(NF)
    t = dev_temporal(torch, ctx, kc.CAM5, [fr], [last], cc.TH)[0]
    tm = ref.temporal_walk(kc.CAM5, fr, last, cc.TH)
    for k in ("temp_flag", "n_temp", "stats", "last_observed", "last_valid", "last_desc"):
        assert np.array_equal(np.asarray(t[k]), np.asarray(tm[k])), ("temporal", NF, k)
    assert np.allclose(t["last_pt"], tm["last_pt"], rtol=0, atol=1e-9)


def test_above_the_capacity_is_an_error_and_writes_nothing(gpu):
    torch, ctx = gpu
    NF = api.STEREO_WALK_MAX + 1
    mean, cov = kc.mk_map(cc.MAP_MOVE)
    fr = generated(NF)
    a = stacked(torch, [fr], [2])
    out = dict({k: torch.full((1, NF), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for k in LISTS + ("feat_new",)},
               new_pos=torch.full((1, NF, 3), -7.5, dtype=torch.float64, device="cuda"), pts0=torch.full((1, NF, 3), -7.5, dtype=torch.float64, device="cuda"),
               n_new=torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), stats=torch.full((1, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
    with pytest.raises(api.GLError, match="GL_STEREO_WALK_MAX"):
        api.create_stereo_points(ctx, gmm_of(ctx, mean, cov), api.Camera(**kc.CAM5), api.Params(), a, 50, 1, 1.5, out=out)
    torch.cuda.synchronize()
    for k, t in out.items():
        v = t.cpu().numpy()
        assert (v == (-7.5 if v.dtype == f64 else 0x5A5A5A5A)).all(), k
    last = {k: T(torch, v[None]) for k, v in cc.last_rows(NF).items()}
    before = {k: v.cpu().numpy() for k, v in last.items()}
    with pytest.raises(api.GLError, match="GL_STEREO_WALK_MAX"):
        api.create_temporal_points(ctx, api.Camera(**kc.CAM5), {k: T(torch, fr[k][None]) for k in api.TEMPORAL_IN_DTYPES}, last, 1.5)
    torch.cuda.synchronize()
    for k, v in last.items():
        assert np.array_equal(v.cpu().numpy(), before[k]), k


# ---- a random key-frame on the real map ---------------------------------------------------------------------------------------------------
def random_key_frame(torch, ctx, g, cam, mean, cov, gt, NF, seed, k=5):
    f = synth.synth_frame(mean, cov, synth.gt_row_to_Tcw(gt[(seed * 37) % gt.shape[0]]), cam, NF, seed, outlier_frac=0.1)
    rng = np.random.default_rng(seed)
    u, v, ur = f["obs"].T
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where((ur >= 0) & (u - ur > 0), cam.bf / (u - ur), -1.0).astype(f32)
    pose = f["pose_gt"]
    cand, ncand, _, _ = g.search2d(cam, T(torch, pose[None]), T(torch, np.ascontiguousarray(f["obs"][None, :, :2])), k=k)
    torch.cuda.synchronize()
    octv = f["octave"].astype(np.int32)
    octv[rng.uniform(size=NF) < 0.02] = -1
    return dict(pose=pose, feat_uv=np.ascontiguousarray(f["obs"][:, :2]), feat_ur=ur.astype(f32), feat_depth=depth, feat_oct=octv, cand=cand[0].cpu().numpy(),
                ncand=ncand[0].cpu().numpy(), held=rng.choice(np.array([0, 1, 2], np.uint8), NF, p=[0.5, 0.35, 0.15]))


def test_random_key_frame_on_the_map(gpu, map_v1, gt_sync):
    """NF = 1 200 on map_v1, th_depth as frame::th_depth (35 bf / fx): the walk held to the model run on the DEVICE's own per-feature check
    results - which isolates the walk, so no feature is excluded"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam = api.Camera()
    g = gmm_of(ctx, mean, cov)
    camd = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, width=cam.width, height=cam.height)
    fr = random_key_frame(torch, ctx, g, cam, mean, cov, gt_sync["V1_01_easy"], 1200, 31)
    th = f32(35.0 * cam.bf / cam.fx)
    for check_depth in (1, 0):
        o = dev_stereo(torch, ctx, g, camd, [fr], [4], 9000, check_depth, th)[0]
        s, comp = split_route(torch, ctx, g, camd, [fr], [o["pts0"]], [4], 9000, check_depth, th)
        same_bits(o, s[0], ("random", check_depth))
        m = ref.stereo_walk(camd, fr, ref.check_table(comp[0], np.zeros((1200, 3))), 9000, check_depth, th, 4)
        assert np.allclose(o["pts0"], m["pts0"], rtol=0, atol=1e-9)
        print("pts0: rows whose bits differ from the numpy model's", int((o["pts0"] != m["pts0"]).any(1).sum()), "max", float(np.abs(o["pts0"] - m["pts0"]).max()))
        st = o["stats"]
        print("random key-frame, check_depth", check_depth, "stats", st.tolist(), "accepted with a component", int((o["new_assoc"] >= 0).sum()))
        assert st[0] > 800 and st[3] > 0 and (o["new_assoc"] >= 0).sum() > 0 and (o["new_assoc"] < 0).sum() > 0 and st[5] == check_depth


# ---- gl_create_temporal_points --------------------------------------------------------------------------------------------------------------
def dev_temporal(torch, ctx, cam, frames, lasts, th):
    fr = {k: T(torch, np.stack([f[k] for f in frames])) for k in api.TEMPORAL_IN_DTYPES}
    last = {k: T(torch, np.stack([l[k] for l in lasts])) for k in api.TEMPORAL_LAST_DTYPES}
    r = api.create_temporal_points(ctx, api.Camera(**cam), fr, last, float(th))
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in dict(r, **last).items()}
    return [dict({k: h[k][b] for k in h if k != "n_temp"}, n_temp=int(h["n_temp"][b])) for b in range(len(frames))]


@pytest.mark.parametrize("name", cc.TEMPORAL)
def test_temporal_case(gpu, name):
    torch, ctx = gpu
    c = cc.CASES[name]
    before = cc.last_rows(c.NF)
    o = dev_temporal(torch, ctx, c.cam, [c.fr], [before], c.th)[0]
    check_temporal(c, o, before)
    # and in the middle of three frames of a wider shape
    NF = c.NF + 9
    frames = [padded(cc.CASES["tmp_held"].fr, NF, 0), padded(c.fr, NF, 4), padded(cc.CASES["tmp_outlier_0_1"].fr, NF, NF - 3)]
    o3 = dev_temporal(torch, ctx, c.cam, frames, [cc.last_rows(NF)] * 3, c.th)[1]
    for k in ("temp_flag", "last_valid", "last_observed", "last_desc"):
        assert o3[k][4:4 + c.NF].tobytes() == o[k].tobytes(), (name, k)
    assert o3["n_temp"] == o["n_temp"] and np.array_equal(o3["stats"], o["stats"])
    made = o["temp_flag"] != 0
    assert o3["last_pt"][4:4 + c.NF][made].tobytes() == o["last_pt"][made].tobytes()
    rest = np.ones(NF, bool)
    rest[4:4 + c.NF] = False
    for k, v in cc.last_rows(NF).items():
        assert np.array_equal(o3[k][rest], v[rest]), (name, k, "a padding slot's row changed")


def test_temporal_arrays_feed_the_chain(gpu):
    """a tracked frame whose last frame holds temporal points: the last-frame arrays with those rows made by gl_create_temporal_points
    give gl_track_frame_chain the bits the arrays made on the host give it"""
    from tests.test_gpu_chain import pack
    torch, ctx = gpu
    cam = api.Camera()
    camd = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
    frames = [synth.synth_chain_frame(600, 500, 1200, 7100 + b, cam, temporal_frac=0.3) for b in range(2)]
    NL = 500
    host, ins, lasts = [], [], []
    for f in frames:
        temporal = f["last_observed"] == 0
        assert temporal.sum() > 50
        X = f["last_pt"]  # (the last frame is at the identity)
        uv = np.stack([cam.fx * X[:, 0] / X[:, 2] + cam.cx, cam.fy * X[:, 1] / X[:, 2] + cam.cy], 1)
        outlier = (np.arange(NL) % 7 == 3).astype(np.uint8)
        fr = dict(pose=f["pose_lw"].astype(f64), feat_uv=uv, feat_depth=X[:, 2].astype(f32), feat_oct=f["last_oct"].astype(np.int32),
                  held=np.where(temporal, np.where(np.arange(NL) % 2 == 0, 0, 2), 1).astype(np.uint8), last_outlier=outlier, feat_desc=f["last_desc"].astype(np.uint8))
        # the rows of the slots without a key-point as a host leaves them before the call: whatever was there
        last = dict(last_pt=np.where(temporal[:, None], -3.25, X), last_observed=np.where(temporal, 9, f["last_observed"]).astype(np.uint8),
                    last_valid=np.where(temporal, 9, f["last_valid"]).astype(np.uint8), last_desc=np.where(temporal[:, None], 0x3C, f["last_desc"]).astype(np.uint8))
        m = ref.temporal_walk(camd, fr, last, f32(1e9))  # (no break: every slot with depth is walked)
        assert np.array_equal(m["temp_flag"] != 0, temporal)
        host.append(dict(f, **{k: m[k] for k in api.TEMPORAL_LAST_DTYPES}))
        ins.append(fr)
        lasts.append(last)
    a_host = pack(torch, host)
    a_dev = pack(torch, host)
    last_dev = {k: T(torch, np.stack([l[k] for l in lasts])) for k in api.TEMPORAL_LAST_DTYPES}
    r = api.create_temporal_points(ctx, cam, {k: T(torch, np.stack([f[k] for f in ins])) for k in api.TEMPORAL_IN_DTYPES}, last_dev, 1e9)
    a_dev.update(last_dev)
    torch.cuda.synchronize()
    assert r["n_temp"].cpu().tolist() == [int((f["last_observed"] == 0).sum()) for f in frames]
    for k in api.TEMPORAL_LAST_DTYPES:
        d, h = a_dev[k].cpu().numpy(), a_host[k].cpu().numpy()
        print(k, "device rows equal to the host's:", bool(d.tobytes() == h.tobytes()))
    outs = []
    for a in (a_host, a_dev):
        o = api.track_frame_chain(ctx, cam, api.Params(), a, th_mm=7.0, th_local=3.0, nn_ratio=0.8, mono=False)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    assert sorted(outs[0]) == sorted(outs[1])
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


# ---- the composite on the resident map ------------------------------------------------------------------------------------------------------
def key_frame_scene(map_v1, gt_sync):
    """tests/map_grow_scenes.geo_scene with its key-frame handed over new; a third of the slots that held a point are null now and a
    sixth hold a temporal point (which the map does not know), so that the walk has points to make"""
    from tests import map_grow_scenes as GS
    sc = GS.geo_scene(*map_v1, gt_sync["V1_01_easy"])
    K = sc["kf_row"]
    m0, ba0 = GS.strip_key_frame(sc["m"], sc["ba"], K)
    cam = api.Camera()
    row = m0["kf_mp"][K].copy()
    had = np.nonzero(row >= 0)[0]
    held = np.where(row >= 0, 1, 0).astype(np.uint8)
    held[had[0::3]] = 0
    held[had[1::6]] = 2
    row[held != 1] = -1
    m0["kf_mp"][K] = row
    u, ur = ba0["kf_uvr"][K][:, 0], ba0["kf_uvr"][K][:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where((ur >= 0) & (u - ur > 0), cam.bf / (u - ur), -1.0).astype(f32)
    return sc, m0, ba0, K, held, depth, cam


def host_key_frame(torch, ctx, g, cam, md, bd, rk, kf_desc, sizes, K, held, depth, th, k=5):
    """the route the composite replaces: search2d, the tables read back, the split route, the lists uploaded, map_add, the refresh"""
    from tests.test_gpu_map_grow import refresh
    NMP = sizes[0]
    camd = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
    uvr = bd["kf_uvr"][K].cpu().numpy()
    pose = bd["kf_pose"][K].cpu().numpy()
    cand, ncand, _, _ = g.search2d(cam, T(torch, pose[None]), T(torch, uvr[None, :, :2]), k=k)
    torch.cuda.synchronize()
    fr = dict(pose=pose, feat_uv=np.ascontiguousarray(uvr[:, :2]), feat_ur=uvr[:, 2].astype(f32), feat_depth=depth, feat_oct=bd["kf_oct"][K].cpu().numpy(),
              cand=cand[0].cpu().numpy(), ncand=ncand[0].cpu().numpy(), held=held)
    pts0 = ref.stereo_walk(camd, fr, ref.check_table(-np.ones(len(held), np.int32), np.zeros((len(held), 3))), NMP, 1, th, K)["pts0"]
    w = split_route(torch, ctx, g, camd, [fr], [pts0], [K], NMP, 1, th)[0][0]
    t = lambda a, dt=np.int32: T(torch, np.asarray(a, dt))
    r = map_grow.map_add(ctx, md, bd, sizes, new_mp=dict(pos=t(w["new_pos"], f64), assoc=t(w["new_assoc"]), ref_kf=t(w["new_ref_kf"])), new_kf=t([K]),
                         attach=dict(mp=t(w["att_mp"]), kf=t(w["att_kf"]), feat=t(w["att_feat"])), mp_ref_kf=rk)
    if not r["status"]:
        refresh(ctx, md, bd, rk, kf_desc, r["sizes"])
    return r, w


def _resident(torch, md, bd, rk):
    torch.cuda.synchronize()
    return dict({"map." + k: v.cpu().numpy() for k, v in md.items() if hasattr(v, "cpu")}, **{"ba." + k: v.cpu().numpy() for k, v in bd.items() if hasattr(v, "cpu")},
                mp_ref_kf=rk.cpu().numpy())


def test_composite_equals_the_host_route(gpu, map_v1, gt_sync):
    from tests.test_gpu_map_grow import refresh, upload, with_point_arrays
    torch, ctx = gpu
    sc, m0, ba0, K, held, depth, cam = key_frame_scene(map_v1, gt_sync)
    g = gmm_of(ctx, *map_v1)
    th = f32(35.0 * cam.bf / cam.fx)
    NMP, NOBS = len(m0["mp_valid"]), len(m0["obs_kf"])
    kf_desc = T(torch, sc["kf_desc"])
    res = []
    for route in ("host", "device"):
        md, bd, rk, sizes = upload(torch, with_point_arrays(m0, NMP + 400), ba0, sc["mp_ref_kf"], NMP + 400, NOBS + 400)
        refresh(ctx, md, bd, rk, kf_desc, sizes)  # the per-point arrays of the map as it stands
        if route == "host":
            r, w = host_key_frame(torch, ctx, g, cam, md, bd, rk, kf_desc, sizes, K, held, depth, th)
        else:
            r = map_grow.process_key_frame_from_map(ctx, g, cam, api.Params(), md, bd, dict(desc=kf_desc), K, T(torch, depth), T(torch, held), float(th), sizes=sizes,
                                                    mp_ref_kf=rk)
            assert r["n_new"] == len(w["new_feat"]) and np.array_equal(r["feat_new"].cpu().numpy(), w["feat_new"]) and np.array_equal(r["stats"].cpu().numpy(), w["stats"])
        assert r["status"] == 0
        res.append((r["sizes"], r["n_attached"], r["n_skipped"], _resident(torch, md, bd, rk)))
    print("key-frame", K, "new points", len(w["new_feat"]), "stats", w["stats"].tolist(), "sizes", res[0][0])
    assert len(w["new_feat"]) > 20 and (w["new_assoc"] >= 0).any() and w["stats"][3] > 0
    assert res[0][:3] == res[1][:3] and res[0][1] == len(w["new_feat"])
    # (update_map_points on the new rows alone = on every row: the old rows' inputs have not changed)
    for k in res[0][3]:
        assert res[0][3][k].tobytes() == res[1][3][k].tobytes(), k


def test_composite_after_a_truncation_changes_nothing(gpu, map_v1, gt_sync):
    from tests.test_gpu_map_grow import refresh, upload, with_point_arrays
    torch, ctx = gpu
    sc, m0, ba0, K, held, depth, cam = key_frame_scene(map_v1, gt_sync)
    g = gmm_of(ctx, *map_v1)
    NMP, NOBS = len(m0["mp_valid"]), len(m0["obs_kf"])
    kf_desc = T(torch, sc["kf_desc"])
    for caps, bit in (((NMP + 3, NOBS + 400), map_grow.GROW_MP_TRUNCATED), ((NMP + 400, NOBS + 3), map_grow.GROW_OBS_TRUNCATED)):
        md, bd, rk, sizes = upload(torch, with_point_arrays(m0, caps[0]), ba0, sc["mp_ref_kf"], *caps)
        refresh(ctx, md, bd, rk, kf_desc, sizes)
        before = _resident(torch, md, bd, rk)
        r = map_grow.process_key_frame_from_map(ctx, g, cam, api.Params(), md, bd, dict(desc=kf_desc), K, T(torch, depth), T(torch, held), 35.0 * cam.bf / cam.fx,
                                                sizes=sizes, mp_ref_kf=rk)
        assert r["status"] & bit and r["sizes"] == sizes and r["n_new"] > 3
        after = _resident(torch, md, bd, rk)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), (k, bit)
