"""gl_map_stats_track, gl_map_stats_new_points, gl_map_cand_append, gl_map_stats_merge and gl_cull_map_points against the sequential
model of tests/map_stats_ref.py and the declared outputs of tests/map_stats_cases.py: integers only, so every array, list, count and
result is compared exactly, and GUARD words behind every output array must keep their sentinel.  The expected output always comes from
the model or the declaration, never from the device."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api, map_grow, map_stats
from tests import local_map_scenes as LS
from tests import map_edit_ref as E
from tests import map_edit_scenes as ES
from tests import map_grow_scenes as GS
from tests import map_stats_cases as SC
from tests import map_stats_ref as R
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.gpu_helpers import stop_on_device_error, to_dev  # noqa: F401 (the fixture is autouse)

pytestmark = pytest.mark.gpu

SENT, NGUARD = -9, 8


class Guarded:
    """int32 device arrays with NGUARD sentinel words behind each: .t[name] is the view the call gets, check() the guards"""

    def __init__(self, torch, **arrays):
        self.full, self.t, self.n = {}, {}, {}
        for k, a in arrays.items():
            a = np.asarray(a, np.int32).ravel()
            self.full[k] = torch.from_numpy(np.concatenate([a, np.full(NGUARD, SENT, np.int32)])).cuda()
            self.t[k], self.n[k] = self.full[k][:len(a)], len(a)

    def host(self, k):
        return self.full[k].cpu().numpy()[:self.n[k]]

    def check(self):
        for k, f in self.full.items():
            assert (f.cpu().numpy()[self.n[k]:] == SENT).all(), "written behind %s" % k


def make_stats(torch, visible, found, ref_idx, kf_idx=None, cand=(), cand_cap=None, NMPcap=None):
    """-> (Guarded, the stats dict on its views): the counters padded with sentinels to NMPcap rows, the list to cand_cap entries"""
    n = len(visible)
    NMPcap = n if NMPcap is None else NMPcap
    cand = np.asarray(cand, np.int32)
    cand_cap = len(cand) if cand_cap is None else cand_cap
    pad = lambda a, m: np.concatenate([np.asarray(a, np.int32), np.full(m - len(a), SENT, np.int32)])
    g = Guarded(torch, visible=pad(visible, NMPcap), found=pad(found, NMPcap), ref_idx=pad(ref_idx, NMPcap), cand=pad(cand, cand_cap), n_cand=[len(cand)])
    st = dict(g.t)
    st["kf_idx"] = None if kf_idx is None else torch.from_numpy(np.asarray(kf_idx, np.int32)).cuda()
    return g, st


def cull_outputs(torch, cap):
    return Guarded(torch, rm_mp=np.full(cap, SENT), n_rm=[SENT], verdict=np.full(cap, SENT), result=np.full(4, SENT))


def device_cull(torch, ctx, m, ba, c, cand, kf_row, cand_cap=None):
    """gl_cull_map_points on a fresh upload -> (verdict, the list afterwards, rm_mp, result); the map, the counters and the guards checked"""
    md, bd = to_dev(torch, {k: m[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}), to_dev(torch, {k: ba[k] for k in ("kf_uvr", "obs_feat")})
    g, st = make_stats(torch, c["visible"], c["found"], c["ref_idx"], c.get("kf_idx"), cand, cand_cap)
    cap = g.n["cand"]
    o = cull_outputs(torch, cap)
    def call(torch, ctx):
        map_stats.cull_map_points(ctx, md, bd, st, kf_row, out=o.t)
        torch.cuda.synchronize()
    run(call, torch, ctx)
    g.check()
    o.check()
    n = len(cand)
    kept, removed, erased, status = o.host("result").tolist()
    assert int(g.host("n_cand")[0]) == kept and int(o.host("n_rm")[0]) == removed and kept + removed + erased == n
    assert (o.host("verdict")[n:] == SENT).all() and (o.host("rm_mp")[removed:] == SENT).all()
    for k in md:  # the map and the counters are not written
        assert np.array_equal(md[k].cpu().numpy(), np.asarray(m[k])), k
    for k in ("visible", "found", "ref_idx"):
        assert np.array_equal(g.host(k)[:len(c[k])], np.asarray(c[k], np.int32)), k
    return o.host("verdict")[:n].tolist(), g.host("cand")[:kept].tolist(), o.host("rm_mp")[:removed].tolist(), [kept, removed, erased, status]


# ---- the cull: the hand-built cases

@pytest.mark.parametrize("variant", ["rows", "shifted"])
@pytest.mark.parametrize("name", list(SC.LISTS))
def test_cull_cases(gpu, name, variant):
    torch, ctx = gpu
    cand, verdict, kept, rm = SC.LISTS[name]
    sc = SC.cull_scene(variant)
    v, k, r, res = device_cull(torch, ctx, sc["m"], sc["ba"], sc, cand, SC.KF_ROW, cand_cap=len(cand) + 3)
    assert v == verdict and k == kept and r == rm, (name, v, k, r)
    assert res == [len(kept), len(rm), len(cand) - len(kept) - len(rm), R.STATUS_BAD_ROW if name in SC.BAD_ROW_LISTS else 0]


def test_cull_wide_ages_are_subtracted_in_64_bits(gpu):
    torch, ctx = gpu
    cand, verdict, kept, rm = SC.WIDE_LIST
    sc = SC.cull_scene("wide")
    v, k, r, res = device_cull(torch, ctx, sc["m"], sc["ba"], sc, cand, SC.KF_ROW)
    assert v == verdict and k == kept and r == rm and res == [2, 0, 2, 0]


# ---- the cull at the wave, workgroup and SCAN_TILE edges

@functools.lru_cache(maxsize=None)
def small_scene():
    return ES.scene("small")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097])
def test_cull_sizes(gpu, n):
    torch, ctx = gpu
    sc = small_scene()
    rng = np.random.default_rng(4200 + n)
    c = SC.random_case(sc, rng, n)
    if n:
        c["cand"] = rng.integers(0, len(sc["m"]["mp_valid"]), n).astype(np.int32)  # (few duplicates: the verdicts stay spread)
        c["cand"][rng.integers(0, n, max(n // 50, 1))] = c["cand"][0]
    M = R.Model(sc["m"], sc["ba"]).set_stats(c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["cand"])
    verdict, removed = M.remove_map_points(c["kf_row"])
    for t0 in range(0, n - 63, 1024):  # every tile holds kept and erased entries
        tile = np.array(verdict[t0:t0 + 1024])
        assert (tile == R.KEPT).any() and (tile != R.KEPT).any() and np.isin(tile, (R.RATIO, R.YOUNG_FEW)).any(), t0
    v, k, r, res = device_cull(torch, ctx, sc["m"], sc["ba"], c, c["cand"], c["kf_row"], cand_cap=n + 5)
    assert v == verdict and k == M.cand and r == removed, n
    assert res[:3] == [len(M.cand), len(removed), n - len(M.cand) - len(removed)]


# ---- append

def test_cand_append_below_at_and_above_the_capacity(gpu):
    torch, ctx = gpu
    T = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    for form in ("list", "list_count", "range", "range_count"):
        for n, fits in ((5, True), (6, True), (7, False)):
            g, st = make_stats(torch, [1], [1], [-1], cand=[40, 41, 42, 43], cand_cap=10)
            rows = np.arange(100, 100 + n + 2).astype(np.int32)
            count = T([n]) if form.endswith("count") else None
            host_n = n + 2 if count is not None else n  # (the device count clamps the host's)
            def call(torch, ctx):
                if form.startswith("list"):
                    return map_stats.map_cand_append(ctx, st, rows=T(rows), n=host_n, n_dev=count).cpu().numpy().tolist()
                return map_stats.map_cand_append(ctx, st, first=100, n=host_n, n_dev=count).cpu().numpy().tolist()
            res = run(call, torch, ctx)
            g.check()
            want = [40, 41, 42, 43] + (list(range(100, 100 + n)) if fits else [])
            assert res == [4 + n, 0 if fits else R.CAND_TRUNCATED], (form, n, res)
            assert int(g.host("n_cand")[0]) == len(want) and g.host("cand")[:len(want)].tolist() == want
            assert (g.host("cand")[len(want):] == SENT).all(), (form, n)


# ---- new points

@pytest.mark.parametrize("table", [False, True])
def test_new_points_up_to_and_across_the_capacity(gpu, table):
    torch, ctx = gpu
    NMPcap, NKF = 16, 6
    kf_idx = [10, 11, 13, 14, 17, 18] if table else None
    idx = lambda k: -1 if not 0 <= k < NKF else (kf_idx[k] if table else k)
    ref_kf = np.array([2, -1, NKF, 5, 0, 3, 4, 1], np.int32)
    for first, n, count in ((10, 6, None), (12, 6, None), (10, 8, 6), (12, 8, 6), (3, 0, None)):
        g, st = make_stats(torch, [7] * NMPcap, [8] * NMPcap, [9] * NMPcap, kf_idx)
        def call(torch, ctx):
            nd = None if count is None else torch.tensor([count], dtype=torch.int32).cuda()
            return int(map_stats.map_stats_new_points(ctx, st, NKF, first, torch.from_numpy(ref_kf[:n].copy()).cuda(), n_dev=nd).cpu()[0])
        status = run(call, torch, ctx)
        g.check()
        k = n if count is None else count
        vis, fnd, ref = [7] * NMPcap, [8] * NMPcap, [9] * NMPcap
        for j in range(k):
            if first + j < NMPcap:
                vis[first + j], fnd[first + j], ref[first + j] = 1, 1, idx(int(ref_kf[j]))
        assert status == (R.MP_TRUNCATED if first + k > NMPcap else 0), (first, n, count)
        assert g.host("visible").tolist() == vis and g.host("found").tolist() == fnd and g.host("ref_idx").tolist() == ref, (first, n, count)


# ---- track

def device_track(torch, ctx, g, st, NMP, a, with_counts2=True):
    d = to_dev(torch, a)
    def call(torch, ctx):
        map_stats.map_stats_track(ctx, st, NMP, d["feat_mp"], d["match_local"], d["outlier"], d["inview"], d["local_mp"], d["n_local_mp"],
                                  d["counts2"] if with_counts2 else None)
        torch.cuda.synchronize()
    run(call, torch, ctx)
    g.check()
    return g.host("visible").tolist(), g.host("found").tolist()


def test_track_case(gpu):
    torch, ctx = gpu
    t, a = SC.TRACK, SC.track_arrays()
    NMP = t["NMP"]
    g, st = make_stats(torch, [1] * NMP, [1] * NMP, [-1] * NMP, NMPcap=NMP + 2)
    vis, fnd = device_track(torch, ctx, g, st, NMP, a)
    assert vis[:NMP] == t["visible_out"] and fnd[:NMP] == t["found_out"] and vis[NMP:] == [SENT] * 2 and fnd[NMP:] == [SENT] * 2
    vis2, fnd2 = device_track(torch, ctx, g, st, NMP, a)  # a second call accumulates onto the first
    assert vis2[:NMP] == [2 * v - 1 for v in t["visible_out"]] and fnd2[:NMP] == [2 * v - 1 for v in t["found_out"]]
    # counts2 NULL: every frame tracked, the lost frame's arrays count too (they equal frame 0's)
    g, st = make_stats(torch, [1] * NMP, [1] * NMP, [-1] * NMP)
    vis3, fnd3 = device_track(torch, ctx, g, st, NMP, a, with_counts2=False)
    ref = R.track(np.ones(NMP, np.int32), np.ones(NMP, np.int32), NMP, **dict(a, counts2=None))
    assert vis3 == ref[0].tolist() and fnd3 == ref[1].tolist() and vis3 != t["visible_out"]
    # a table of fewer rows: what lies at or above NMP counts nothing and is not written
    g, st = make_stats(torch, [1] * NMP, [1] * NMP, [-1] * NMP)
    vis4, fnd4 = device_track(torch, ctx, g, st, 6, a)
    ref = R.track(np.ones(NMP, np.int32), np.ones(NMP, np.int32), 6, **a)
    assert vis4 == ref[0].tolist() and fnd4 == ref[1].tolist() and vis4[6:] == [1] * 4


@pytest.mark.parametrize("name", ["fallback_one", "plain", "mixed"])
def test_track_on_the_chains_outputs(gpu, name):
    """B = 1, B = 3 and a batch with a lost frame through the real api.track_frame_chain_map: the counters against the model fed the same
    chain outputs and against the outputs copied to the host and incremented in numpy; a second call accumulates"""
    from tests.test_gpu_local_map import lm_dev, pack_chain, TH_LOCAL, TH_MM
    torch, ctx = gpu
    frames, s, lists, KFcap, NPcap = LS.chain_scene(name)
    cam, prm = api.Camera(), api.Params()
    a = {k: v for k, v in pack_chain(torch, frames, NPcap).items() if k not in api.CHAIN_MAP_IGNORED}
    lm, md = lm_dev(torch, s, lists), to_dev(torch, s["map"])
    NMP = len(s["map"]["mp_valid"])
    rng = np.random.default_rng(77)
    vis0, fnd0 = rng.integers(1, 50, NMP).astype(np.int32), rng.integers(1, 20, NMP).astype(np.int32)
    g, st = make_stats(torch, vis0, fnd0, [-1] * NMP, NMPcap=NMP + 7)
    def call(torch, ctx):
        out = map_stats.track_frame_with_stats(ctx, cam, prm, a, md, lm, st, th_mm=TH_MM, th_local=TH_LOCAL, nn_ratio=0.8)
        torch.cuda.synchronize()
        return out
    out = run(call, torch, ctx)
    g.check()
    h = {k: out[k].cpu().numpy() for k in ("feat_mp", "match_local", "outlier", "inview", "counts2")}
    h.update(local_mp=lm["local_mp"].cpu().numpy(), n_local_mp=lm["n_local_mp"].cpu().numpy())
    assert (h["counts2"][:, 3] == 2).sum() == LS.CHAIN_MODES[name].count(2)
    vis, fnd = R.track(vis0, fnd0, NMP, **h)  # the parent's route: the arrays on the host, incremented there
    assert (vis != vis0).sum() > 100 and (fnd != fnd0).sum() > 100
    m, ba = SC.build_map([(int(v), ()) for v in s["map"]["mp_valid"]])
    M = R.Model(m, ba).set_stats(vis0, fnd0, [-1] * NMP)
    R.model_track(M, **h)
    assert M.num_visible == vis.tolist() and M.num_found == fnd.tolist()
    assert M.events["held"] > 0 and M.events["in_view"] > 0 and M.events["found"] > 0 and M.events["matched_local"] > 0
    assert g.host("visible")[:NMP].tolist() == vis.tolist() and g.host("found")[:NMP].tolist() == fnd.tolist()
    assert (g.host("visible")[NMP:] == SENT).all() and (g.host("found")[NMP:] == SENT).all()
    d = to_dev(torch, h)
    def again(torch, ctx):
        map_stats.map_stats_track(ctx, st, NMP, d["feat_mp"], d["match_local"], d["outlier"], d["inview"], d["local_mp"], d["n_local_mp"], d["counts2"])
        torch.cuda.synchronize()
    run(again, torch, ctx)
    vis2, fnd2 = R.track(vis, fnd, NMP, **h)
    assert g.host("visible")[:NMP].tolist() == vis2.tolist() and g.host("found")[:NMP].tolist() == fnd2.tolist()


# ---- merge

def device_merge(torch, ctx, visible, found, NMP, src, tgt, count=None, extra=0):
    g, st = make_stats(torch, visible, found, [-1] * len(visible))
    T = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    s2, t2 = list(src) + [0] * extra, list(tgt) + [1] * extra  # (steps behind the device count: not walked)
    def call(torch, ctx):
        map_stats.map_stats_merge(ctx, st, NMP, T(s2), T(t2), n_dev=None if count is None else T([count]))
        torch.cuda.synchronize()
    run(call, torch, ctx)
    g.check()
    return g.host("visible").tolist(), g.host("found").tolist()


@pytest.mark.parametrize("form", ["host", "count"])
def test_merge_case(gpu, form):
    torch, ctx = gpu
    c = SC.MERGE
    vis, fnd = device_merge(torch, ctx, c["visible"], c["found"], c["NMP"], c["src"], c["tgt"], *((len(c["src"]), 3) if form == "count" else ()))
    assert vis == c["visible_out"] and fnd == c["found_out"]


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2500])
def test_merge_long_chains(gpu, n):
    """the walk across the chunks of 1 024 steps: random steps over few rows, so that targets become sources again and again"""
    torch, ctx = gpu
    rng = np.random.default_rng(900 + n)
    NMP = 300
    vis0, fnd0 = rng.integers(-5, 1000, NMP).astype(np.int32), rng.integers(0, 1000, NMP).astype(np.int32)
    src, tgt = rng.integers(-1, NMP + 1, n), rng.integers(-1, NMP + 1, n)
    src[n // 2:] = tgt[:n - n // 2]  # chains: an earlier step's target is the source
    ref = R.merge(vis0, fnd0, NMP, src, tgt)
    vis, fnd = device_merge(torch, ctx, vis0, fnd0, NMP, src, tgt)
    assert vis == ref[0].tolist() and fnd == ref[1].tolist()


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_merge_on_a_real_fuse(gpu, name):
    """repl_src / repl_tgt and the device count of a real gl_map_fuse: the counters against the model's replaceMapPoint"""
    from tests.test_gpu_map_grow import upload
    torch, ctx = gpu
    sc = ES.scene(name)
    kf, cand, best = GS.fuse_lists(sc, 31)
    m, ba = sc["m"], sc["ba"]
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    rng = np.random.default_rng(5)
    vis0, fnd0 = rng.integers(1, 90, NMP).astype(np.int32), rng.integers(1, 30, NMP).astype(np.int32)
    M = R.Model(m, ba).set_stats(vis0, fnd0, [-1] * NMP)
    _, _, replaced = M.fuse_apply(M.kfs[int(kf)], cand, best)
    assert len(replaced) > 3 and M.events["replace"] == len(replaced)
    md, bd, _, sizes = upload(torch, m, ba, None, NMP, NOBS + len(cand))
    g, st = make_stats(torch, vis0, fnd0, [-1] * NMP)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()
    def call(torch, ctx):
        r = map_grow.map_fuse(ctx, md, bd, kf, T(cand), T(best), sizes=sizes, repl_cap=len(cand))
        src, tgt = torch.full((len(cand),), -1, dtype=torch.int32).cuda(), torch.full((len(cand),), -1, dtype=torch.int32).cuda()
        src[:len(r["repl_src"])], tgt[:len(r["repl_tgt"])] = r["repl_src"], r["repl_tgt"]
        n_dev = torch.tensor([r["n_replaced"]], dtype=torch.int32).cuda()
        map_stats.map_stats_merge(ctx, st, NMP, src, tgt, n_dev=n_dev)
        torch.cuda.synchronize()
        return r
    r = run(call, torch, ctx)
    g.check()
    assert list(zip(r["repl_src"].cpu().tolist(), r["repl_tgt"].cpu().tolist())) == replaced
    assert g.host("visible").tolist() == M.num_visible and g.host("found").tolist() == M.num_found


# ---- the composite and the readers of the edited map

def composite(torch, ctx, sc, c):
    """remove_map_points_from_map on a fresh upload -> (the dict, the device's map dicts after the edit, the Guarded stats)"""
    m, ba = sc["m"], sc["ba"]
    md, bd = to_dev(torch, {k: m[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}), to_dev(torch, {k: ba[k] for k in ("kf_uvr", "kf_oct", "obs_feat", "kf_first")})
    rk = torch.from_numpy(sc["mp_ref_kf"].copy()).cuda()
    g, st = make_stats(torch, c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["cand"], cand_cap=len(c["cand"]) + 4)
    def call(torch, ctx):
        r = map_stats.remove_map_points_from_map(ctx, md, bd, st, c["kf_row"], mp_ref_kf=rk, want_new_pos=True)
        torch.cuda.synchronize()
        return r
    r = run(call, torch, ctx)
    g.check()
    return r, rk, g


@pytest.mark.parametrize("name,n", [("tiny", 40), ("small", 700)])
def test_remove_map_points_from_map_equals_the_model(gpu, name, n):
    torch, ctx = gpu
    sc = ES.scene(name)
    c = SC.random_case(sc, np.random.default_rng(31 + n), n)
    M = R.Model(sc["m"], sc["ba"], sc["mp_ref_kf"]).set_stats(c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["cand"])
    verdict, removed = M.remove_map_points(c["kf_row"])
    assert removed and len(M.cand) > 0 and M.events["invalid_again"] > 0
    rows = M.to_rows()
    r, rk, g = composite(torch, ctx, sc, c)
    nobs = r["remove"]["nobs"]
    dev = dict(mp_valid=r["remove"]["map"]["mp_valid"], kf_valid=r["remove"]["map"]["kf_valid"], kf_mp=r["remove"]["map"]["kf_mp"],
               obs_ptr=r["remove"]["map"]["obs_ptr"], obs_kf=r["remove"]["map"]["obs_kf"][:nobs], obs_feat=r["remove"]["ba"]["obs_feat"][:nobs],
               mp_ref_kf=rk, obs_new_pos=r["remove"]["obs_new_pos"])
    for k, t in dev.items():
        assert np.array_equal(t.cpu().numpy(), rows[k]), (name, k)
    assert r["remove"]["dead_mp"].cpu().tolist() == sorted(removed) and r["remove"]["status"] == 0
    kept = int(g.host("n_cand")[0])
    assert g.host("cand")[:kept].tolist() == M.cand and r["cull"]["verdict"].cpu().numpy()[:n].tolist() == verdict
    assert r["cull"]["rm_mp"].cpu().numpy()[:len(removed)].tolist() == removed and int(r["cull"]["n_rm"].cpu()[0]) == len(removed)


def test_readers_of_the_edited_map(gpu):
    """gl_update_local_map and gl_ba_window_build on the map the composite edited give what they give on the model's rows uploaded"""
    from tests import ba_window_scenes as S
    from tests.test_gpu_ba_window import to_host
    torch, ctx = gpu
    sc = ES.scene("small")
    c = SC.random_case(sc, np.random.default_rng(731), 700)
    M = R.Model(sc["m"], sc["ba"], sc["mp_ref_kf"]).set_stats(c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["cand"])
    M.remove_map_points(c["kf_row"])
    m2, ba2 = E.apply_rows(sc["m"], sc["ba"], M.to_rows())
    r, _, _ = composite(torch, ctx, sc, c)
    NMP, NKF, NFK = len(m2["mp_valid"]), len(m2["kf_valid"]), m2["kf_mp"].shape[1]
    per_point = {k: sc["m"][k] for k in ("mp_pos",) if k in sc["m"]}
    views = []
    for edited in (True, False):
        if edited:
            md = dict(r["remove"]["map"])
            bd = dict(r["remove"]["ba"])
        else:
            md = to_dev(torch, {k: m2[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")})
            bd = to_dev(torch, {k: ba2[k] for k in ("kf_uvr", "kf_oct", "obs_feat", "kf_first")})
        md.update(to_dev(torch, per_point))
        for k in ("kf_pose", "kf_twc", "mp_assoc"):
            if k in sc["ba"]:
                bd[k] = torch.from_numpy(np.ascontiguousarray(sc["ba"][k])).cuda()
        views.append((md, bd))
    rng = np.random.default_rng(3)
    feat_mp = rng.integers(-1, NMP, (2, 200)).astype(np.int32)
    outs = []
    for md, bd in views:
        def call(torch, ctx):
            lists = api.local_map_lists(2, 64, 2048, NKF)
            fm = torch.from_numpy(feat_mp.copy()).cuda()
            api.update_local_map(ctx, {k: md[k] for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")}, fm, lists)
            o = dict(to_host(lists), feat_mp=fm.cpu().numpy())
            if "kf_pose" in bd and "mp_pos" in md:
                caps = dict(Pcap=32, Fcap=128, Lcap=8192, Ocap=65536)
                slab = api.ba_window_slab(1, caps["Pcap"], caps["Fcap"], caps["Lcap"], caps["Ocap"])
                api.ba_window_build(ctx, md, bd, torch.tensor([int(sc["rows"][0])], dtype=torch.int32).cuda(), slab)
                o.update({"win_" + k: v for k, v in to_host(slab).items()})
            torch.cuda.synchronize()
            return o
        outs.append(run(call, torch, ctx))
    assert outs[0]["n_local_mp"].min() > 0
    for k in outs[0]:
        assert np.asarray(outs[0][k]).tobytes() == np.asarray(outs[1][k]).tobytes(), k


# ---- malformed input

def test_malformed_lists_and_csr_are_skipped(gpu):
    """rows out of range in every list, CSR ranges outside [0, NOBS], new_ref_kf out of range: the outputs are as the direct definitions
    of tests/map_stats_ref.py declare them, the guard words behind every output keep their sentinel"""
    from tests import ba_window_scenes as S
    torch, ctx = gpu
    sc = ES.scene("tiny")
    m, ba = {k: np.array(v) for k, v in sc["m"].items()}, {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in sc["ba"].items()}
    S.malform(m, ba, 5)
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    ptr = m["obs_ptr"].astype(np.int64)
    assert ((ptr[:-1] < 0) | (ptr[1:] < ptr[:-1]) | (ptr[1:] > NOBS)).any(), "no CSR range outside [0, NOBS]"
    rng = np.random.default_rng(8)
    c = SC.random_case(dict(m=m, ba=ba), rng, 120)
    c["visible"][:], c["found"][:] = 1, 1  # (the ratio keeps everything: the weights and ages decide)
    bad = np.nonzero((ptr[:-1] < 0) | (ptr[1:] < ptr[:-1]) | (ptr[1:] > NOBS))[0]
    c["cand"][:len(bad[:10])] = bad[:10]
    c["ref_idx"][bad[:10]] = (c["kf_row"] if c["kf_idx"] is None else int(c["kf_idx"][c["kf_row"]])) - 2  # (old enough for the weight to decide)
    c["cand"][10:16] = (-1, NMP, -2 ** 31, 2 ** 31 - 1, NMP + 5, -7)
    verdict, kept, rm, res = R.cull_arrays(m, ba, c["visible"], c["found"], c["ref_idx"], c["kf_idx"], c["kf_row"], c["cand"])
    assert res[3] == R.STATUS_BAD_ROW and R.YOUNG_FEW in verdict and R.KEPT in verdict
    v, k, r, got = device_cull(torch, ctx, m, ba, c, c["cand"], c["kf_row"], cand_cap=125)
    assert v == verdict and k == kept and r == rm and got == res
    # track and merge: rows far outside the table in every list
    t, a = SC.TRACK, SC.track_arrays()
    for key in ("feat_mp", "local_mp", "match_local"):
        a[key] = a[key].copy()
    a["feat_mp"][0, 2], a["feat_mp"][2, 4], a["local_mp"][0, 1], a["local_mp"][2, 0] = 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -5
    a["match_local"][0, 4], a["match_local"][2, 5], a["n_local_mp"][2] = 2 ** 31 - 1, -2 ** 31, -4
    a["inview"][:] = 1
    ones = np.ones(t["NMP"], np.int32)
    g, st = make_stats(torch, ones, ones, -ones)
    vis, fnd = device_track(torch, ctx, g, st, t["NMP"], a)
    ref = R.track(ones, ones, t["NMP"], **a)
    assert vis == ref[0].tolist() and fnd == ref[1].tolist()
    src, tgt = [0, 2 ** 31 - 1, -2 ** 31, 3, 9], [2 ** 31 - 1, 1, 2, -2 ** 31, 10]
    vis, fnd = device_merge(torch, ctx, list(range(10)), list(range(10)), 10, src, tgt)
    assert vis == list(range(10)) and fnd == list(range(10))
