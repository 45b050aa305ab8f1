"""gl_update_local_map (Tracking::updateLocalMap, tracking.cpp:119-207, on the device) against tests/local_map_ref.py - every output is
an integer, so equality is exact - and gl_track_frame_chain_map against the sequence it replaces: gl_track_frame_chain_front -> the
restatement + a host gather -> gl_track_frame_chain_back, bit for bit on every output.  The scenes and the conditions they meet:
tests/local_map_scenes.py, tests/test_local_map_ref.py."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import chain_glue as G
from tests import local_map_ref as R
from tests import local_map_scenes as S
from tests.chain_glue import TH_LOCAL, TH_MM
from tests.gpu_helpers import to_dev
from tests.test_gpu_chain import pack

pytestmark = pytest.mark.gpu

MAP_KEYS = ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")
POINT_KEYS = api.MAP_VIEW_POINT_KEYS
CHAIN_OUT = ("pose", "pose_mm", "match_last", "match_kf", "match_local", "outlier", "counts", "counts2", "drop_src", "drop_kf", "inview")
LIST_KEYS = ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "kf_count", "status")


def to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def device_update(torch, ctx, m, feat_mp, lists, md=None):
    md = to_dev(torch, m, MAP_KEYS) if md is None else md
    fm, ld = torch.from_numpy(feat_mp.copy()).cuda(), to_dev(torch, lists)
    api.update_local_map(ctx, md, fm, ld)
    torch.cuda.synchronize()
    return fm.cpu().numpy(), to_host(ld)


def assert_same(dev, ref, what):
    fm_d, l_d = dev
    fm_r, l_r = ref
    assert np.array_equal(fm_d, fm_r), (what, "feat_mp")
    for k in l_r:
        assert np.array_equal(l_d[k], l_r[k]), (what, k, np.nonzero(np.atleast_1d(l_d[k] != l_r[k]).reshape(len(l_r[k]), -1).any(1))[0][:8])


@pytest.mark.parametrize("name", list(S.UPDATE_SCENES))
def test_update_local_map_equals_the_restatement(gpu, name):
    """tiny maps, a EuRoC-sized one (B = 1 and B = 256) and maps on either side of each LDS bound (counters: 4 096 key-frames, mask:
    1 048 576 map points - above a bound that array lives in global memory): feat_mp, the lists behind their sentinels, the true
    counts, ref_kf, kf_count and status all equal; the same bytes when run again; and without the optional kf_count"""
    torch, ctx = gpu
    m, feat_mp, lists = S.update_scene(name)
    ref = R.update_local_map(m, feat_mp, lists)
    md = to_dev(torch, m, MAP_KEYS)
    dev = device_update(torch, ctx, m, feat_mp, lists, md)
    assert_same(dev, ref, name)
    again = device_update(torch, ctx, m, feat_mp, lists, md)
    assert again[0].tobytes() == dev[0].tobytes() and all(again[1][k].tobytes() == dev[1][k].tobytes() for k in dev[1])
    no_count = {k: v for k, v in lists.items() if k != "kf_count"}
    dev2 = device_update(torch, ctx, m, feat_mp, no_count, md)
    assert_same(dev2, (ref[0], {k: v for k, v in ref[1].items() if k != "kf_count"}), name + " without kf_count")
    if S.UPDATE_SCENES[name][4] >= 16:
        assert (ref[1]["status"] == R.KEPT).any() and (ref[1]["status"] == 0).any()


def test_update_local_map_all_valid_by_null_pointers(gpu):
    torch, ctx = gpu
    m, feat_mp, lists = S.update_scene("small")
    m = dict(m, mp_valid=None, kf_valid=None)
    assert_same(device_update(torch, ctx, m, feat_mp, lists), R.update_local_map(m, feat_mp, lists), "null validity")


@pytest.mark.parametrize("KFcap,NPcap", [(5, 100), (1, 1), (128, 700), (7, 4096)])
def test_update_local_map_truncation(gpu, KFcap, NPcap):
    """capacities below the lists: the lowest rows are kept, the true counts reported, the status bits set, nothing written past a capacity"""
    torch, ctx = gpu
    seed, NMP, NKF, NFK, B, NF, _, _ = S.UPDATE_SCENES["small"]
    m, feat_mp, _ = S.update_scene("small")
    lists = S.previous_lists(B, NKF, NMP, KFcap, NPcap)
    ref = R.update_local_map(m, feat_mp, lists)
    assert (ref[1]["status"] & R.MP_TRUNCATED).any() == (NPcap < 4096) and (ref[1]["status"] & R.KF_TRUNCATED).any() == (KFcap < 128)
    assert_same(device_update(torch, ctx, m, feat_mp, lists), ref, (KFcap, NPcap))


@pytest.mark.parametrize("name", ["small", "kf_over_bound"])
def test_update_local_map_malformed_input_is_skipped(gpu, name):
    """rows outside the tables in feat_mp, kf_mp, obs_kf and obs_ptr (on the LDS path and on the global-counter path): skipped as the
    restatement skips them, every output still exact behind its sentinels"""
    torch, ctx = gpu
    m, feat_mp, lists = S.update_scene(name)
    NMP, NKF, NFK, NOBS = R._sizes(m)
    rng = np.random.default_rng(5)
    m = {k: (v.copy() if v is not None else None) for k, v in m.items()}
    bad = np.array([NMP, NMP + 5, 2 ** 31 - 1, -2, -2 ** 31], np.int64)
    at = rng.uniform(size=feat_mp.shape) < 0.05
    feat_mp[at] = rng.choice(bad, int(at.sum()))
    at = rng.uniform(size=m["kf_mp"].shape) < 0.02
    m["kf_mp"][at] = rng.choice(bad, int(at.sum()))
    at = rng.uniform(size=NOBS) < 0.02
    m["obs_kf"][at] = rng.choice(np.array([NKF, NKF + 3, 2 ** 31 - 1, -1, -2 ** 31], np.int64), int(at.sum()))
    pts = rng.choice(NMP, 60, replace=False)
    m["obs_ptr"][pts] = rng.choice(np.array([-1, NOBS + 1, 2 ** 31 - 1, -2 ** 31], np.int64), 60)  # (ranges that start or end outside [0, NOBS], or run backwards)
    held = feat_mp[(feat_mp >= 0) & (feat_mp < NMP)]
    m["obs_ptr"][held[:3]] = NOBS + 7  # ... of points some feature really holds
    ref = R.update_local_map(m, feat_mp, lists)
    assert (ref[1]["status"] == 0).any()
    assert_same(device_update(torch, ctx, m, feat_mp, lists), ref, name)


def test_update_local_map_arguments(gpu):
    """B = 0 is a no-op; bad arguments give GL_ERR_ARG with the entry points' "<function>: <what>" message"""
    torch, ctx = gpu
    m, feat_mp, lists = S.update_scene("tiny")
    md = to_dev(torch, m, MAP_KEYS)
    ld = to_dev(torch, lists)
    before = to_host(ld)
    api.update_local_map(ctx, md, torch.zeros((0, 50), dtype=torch.int32, device="cuda"), {k: v[:0].contiguous() for k, v in ld.items()})
    torch.cuda.synchronize()
    assert all(np.array_equal(before[k], v.cpu().numpy()) for k, v in ld.items())
    fm = torch.from_numpy(feat_mp).cuda()
    for broken, msg in ((dict(md, obs_kf=md["obs_kf"].long()), "int32"), (dict(md, kf_mp=md["kf_mp"].t()), "contiguous"),
                        (dict(md, mp_valid=md["mp_valid"][:-1].contiguous()), "shape"), (dict(md, kf_mp=md["kf_mp"].cpu()), "CUDA")):
        with pytest.raises(AssertionError, match=msg):
            api.update_local_map(ctx, broken, fm, ld)
    with pytest.raises(AssertionError, match="shape"):
        api.update_local_map(ctx, md, fm, dict(ld, ref_kf=ld["ref_kf"][:-1].contiguous()))
    # past the wrapper: the library's own checks
    import ctypes as C
    v, _ = api._map_view(md, False)
    p = api._ptr
    args = lambda **kw: [kw.get("map", C.byref(v)), kw.get("B", 16), kw.get("NF", 50), kw.get("KFcap", 64), kw.get("NPcap", 256), p(fm), p(ld["local_kf"]),
                         p(ld["n_local_kf"]), p(ld["local_mp"]), p(ld["n_local_mp"]), p(ld["ref_kf"]), None, kw.get("status", p(ld["status"]))]
    for kw, msg in ((dict(B=-1), "bad B / NF / KFcap / NPcap"), (dict(KFcap=0), "bad B / NF / KFcap / NPcap"), (dict(status=None), "null buffer"),
                    (dict(map=None), "null argument")):
        assert ctx.lib.gl_update_local_map(ctx.h, *args(**kw)) == -1
        err = ctx.lib.gl_last_error_string().decode()
        assert err.endswith(": " + msg) and "local_map" in err, err
    v.obs_ptr = None
    assert ctx.lib.gl_update_local_map(ctx.h, *args()) == -1 and ctx.lib.gl_last_error_string().decode().endswith("null obs_ptr")


# ---- the chain

def pack_chain(torch, frames, NPcap):
    """the frames' inputs WITHOUT their local maps (the map call makes them): placeholders of NPcap slots where the halves want arrays"""
    B, NL = len(frames), len(frames[0]["last_oct"])
    blank = dict(mp_pos=np.zeros((NPcap, 3)), mp_normal=np.zeros((NPcap, 3)), mp_max_dist=np.zeros(NPcap, np.float32), mp_min_dist=np.zeros(NPcap, np.float32),
                 mp_cand=np.zeros(NPcap, np.uint8), mp_desc=np.zeros((NPcap, 32), np.uint8), last_to_local=-np.ones(NL, np.int32))
    fs = []
    for f in frames:
        g = dict(f)
        g.update(blank)
        if "kf_to_local" in g:
            g["kf_to_local"] = -np.ones(len(f["kf_to_local"]), np.int32)
        fs.append(g)
    return pack(torch, fs)


def lm_dev(torch, s, lists):
    lm = to_dev(torch, lists)
    lm["last_mp"] = torch.from_numpy(np.stack(s["last_mp"])).cuda()
    if s["kf_feat_mp"][0] is not None:
        lm["kf_feat_mp"] = torch.from_numpy(np.stack(s["kf_feat_mp"])).cuda()
    return lm


def run_map_chain(torch, ctx, frames, s, lists, NPcap, md=None, cam=None, prm=None, scale_factor=1.2):
    cam, prm = cam or api.Camera(), prm or api.Params()
    a = pack_chain(torch, frames, NPcap)
    a = {k: v for k, v in a.items() if k not in api.CHAIN_MAP_IGNORED}  # (the call reads none of them)
    lm = lm_dev(torch, s, lists)
    md = to_dev(torch, s["map"]) if md is None else md
    out = api.track_frame_chain_map(ctx, cam, prm, a, md, lm, th_mm=TH_MM, th_local=TH_LOCAL, nn_ratio=0.8, scale_factor=scale_factor)
    torch.cuda.synchronize()
    return to_host(out), {k: v.cpu().numpy() for k, v in lm.items() if k in LIST_KEYS}


def run_halves(torch, ctx, frames, s, lists, NPcap, fit=False):
    """gl_track_frame_chain_front -> (host: feat_mp, tests/local_map_ref.py, gather) -> gl_track_frame_chain_back on the buffers the
    front wrote.  fit: the gathered local map has exactly n_local_mp slots (B = 1 only) instead of NPcap with padding."""
    cam, prm = api.Camera(), api.Params()
    a = pack_chain(torch, frames, NPcap)
    front = api.track_frame_chain_front(ctx, cam, prm, a, th_mm=TH_MM)
    torch.cuda.synchronize()
    fr = to_host(front)
    B = len(frames)
    hs = []
    for b, f in enumerate(frames):
        one = dict(match_last=fr["match_last"][b], match_kf=fr["match_kf"][b] if "match_kf" in fr else -np.ones_like(fr["match_last"][b]),
                   mode=int(fr["counts2"][b, 3]))
        hs.append(S.host_between_halves(s["map"], f, b, s, one, lists, NP="fit" if fit else None))
    assert not fit or B == 1
    fs = []
    for f, h in zip(frames, hs):
        g = dict(f)
        g.update(h["local"])
        fs.append(g)
    a2 = pack(torch, fs)
    front["match_last"].copy_(torch.from_numpy(np.stack([h["match_last"] for h in hs])))
    if "match_kf" in front:
        front["match_kf"].copy_(torch.from_numpy(np.stack([h["match_kf"] for h in hs])))
    out = api.track_frame_chain_back(ctx, cam, prm, a2, front, th_local=TH_LOCAL, nn_ratio=0.8)
    torch.cuda.synchronize()
    out = to_host(out)
    out["feat_mp"] = np.stack([h["feat_mp"] for h in hs])
    ls = {k: np.concatenate([h["lists"][k] for h in hs]) for k in hs[0]["lists"]}
    return out, ls, fs


@pytest.mark.parametrize("name", ["one", "plain", "mixed", "fallback_one", "branches"])
def test_chain_map_equals_front_host_back(gpu, name):
    """plain frames, temporal points, the key-frame fallback and a lost frame, B = 1 and mixed batches: every output of the one call
    equals, bit for bit, the two halves around the host's updateLocalMap with NP = NPcap and the same padding; twice the same bytes"""
    torch, ctx = gpu
    frames, s, lists, KFcap, NPcap = S.chain_scene(name)
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    ref, lr, _ = run_halves(torch, ctx, frames, s, lists, NPcap)
    assert out["counts2"][:, 3].tolist() == S.CHAIN_MODES[name]
    for k in CHAIN_OUT + ("feat_mp",):
        if k in ref:
            assert out[k].tobytes() == ref[k].tobytes(), k
    for k in lr:
        assert np.array_equal(ls[k], lr[k]), k
    tracked = out["counts2"][:, 3] != 2
    assert (out["counts"][tracked, 2] > 0).all() and (ls["status"][tracked] == 0).all() and (ls["status"][~tracked] == R.KEPT).all()
    again, ls2 = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    assert all(again[k].tobytes() == out[k].tobytes() for k in out) and all(ls2[k].tobytes() == ls[k].tobytes() for k in ls)


@pytest.mark.parametrize("name", ["one", "plain", "mixed"])
def test_chain_map_padding_changes_nothing(gpu, name):
    """against the halves run frame by frame on the UNPADDED list (NP = n_local_mp): the padding slots (mp_cand = 0) change no output;
    inview agrees on the list and is 0 on the padding"""
    torch, ctx = gpu
    frames, s, lists, KFcap, NPcap = S.chain_scene(name)
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    for b, f in enumerate(frames):
        sb = dict(s, last_mp=[s["last_mp"][b]], kf_feat_mp=[s["kf_feat_mp"][b]])
        one, l1, fs = run_halves(torch, ctx, [f], sb, {k: v[b:b + 1] for k, v in lists.items()}, NPcap, fit=True)
        n = len(fs[0]["mp_cand"])
        assert n == max(min(int(ls["n_local_mp"][b]), NPcap), 1) and n < NPcap
        for k in CHAIN_OUT + ("feat_mp",):
            if k in one and k != "inview":
                assert out[k][b].tobytes() == one[k][0].tobytes(), (b, k)
        assert np.array_equal(out["inview"][b, :n], one["inview"][0]) and not out["inview"][b, n:].any(), b


def test_chain_map_stages_equal_the_oracle_on_the_device_made_list(gpu, oracle):
    """tests/chain_glue.py::check_chain on the one call's outputs, with the frame's local map = the list the DEVICE made (gathered on
    the host): every stage equals the oracle's function on the inputs the device gave it.  (A scene without invalid map points:
    check_chain knows nothing of clearing.)"""
    torch, ctx = gpu
    cam = api.Camera()
    frames, s, lists, KFcap, NPcap = S.chain_scene("all_valid")
    out, ls = run_map_chain(torch, ctx, frames, s, lists, NPcap)
    n3 = 0
    for b, f in enumerate(frames):
        g = dict(f)
        g.update(R.gather_local_map(s["map"], ls["local_mp"][b], ls["n_local_mp"][b], NPcap, s["last_mp"][b], s["kf_feat_mp"][b]))
        c = G.check_chain(oracle, cam, g, out, b)
        assert c["front"]["mode"] == S.CHAIN_MODES["all_valid"][b]
        n3 += c["n3"]
        r = R.frame_vec(s["map"], out["feat_mp"][b])
        assert np.array_equal(r["local_mp"], ls["local_mp"][b, :ls["n_local_mp"][b]]) and r["ref_kf"] == ls["ref_kf"][b]
    assert n3 > 0


def test_chain_map_arguments(gpu):
    torch, ctx = gpu
    cam, prm = api.Camera(), api.Params()
    frames, s, lists, KFcap, NPcap = S.chain_scene("plain")
    a = {k: v for k, v in pack_chain(torch, frames, NPcap).items() if k not in api.CHAIN_MAP_IGNORED}
    md, lm = to_dev(torch, s["map"]), lm_dev(torch, s, lists)
    for kw, msg in ((dict(a=dict(a, feat_desc=a["feat_desc"][:, :-1].contiguous())), "shape"), (dict(a=dict(a, last_pt=a["last_pt"].float())), "float64"),
                    (dict(md={k: v for k, v in md.items() if k != "mp_desc"}), "missing"), (dict(md=dict(md, mp_pos=md["mp_pos"][:, :2])), "contiguous"),
                    (dict(lm=dict(lm, last_mp=lm["last_mp"][:, :-1].contiguous())), "shape"), (dict(lm=dict(lm, status=lm["status"].cpu())), "CUDA")):
        with pytest.raises(AssertionError, match=msg):
            api.track_frame_chain_map(ctx, cam, prm, kw.get("a", a), kw.get("md", md), kw.get("lm", lm))
    empty = {k: v[:0].contiguous() for k, v in a.items()}
    out = api.track_frame_chain_map(ctx, cam, prm, empty, md, {k: v[:0].contiguous() for k, v in lm.items()})  # B = 0: a no-op
    assert out["match_local"].shape == (0, a["feat_oct"].shape[1])
