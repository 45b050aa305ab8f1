"""gl_map_add and gl_map_fuse against the sequential object model of tests/map_grow_ref.py: integers only, so every array, result, list
and obs_new_pos is compared byte for byte and every entry behind an output's contents must keep its sentinel; the readers of the
resident map on the device-grown arrays; one composed mapping pass against the model's edits uploaded.  The scenes and the conditions
they meet: tests/map_grow_scenes.py, tests/test_map_grow_ref.py.  The expected output always comes from the model, never from the
device."""
import ctypes as C

import numpy as np
import pytest

from gmmloc_amd import api, map_grow
from tests import ba_window_ref as R
from tests import ba_window_scenes as S
from tests import map_edit_ref as E
from tests import map_edit_scenes as ES
from tests import map_grow_ref as G
from tests import map_grow_scenes as GS
from tests import map_point_ref as MP
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.gpu_helpers import stop_on_device_error, to_dev  # noqa: F401 (the fixture is autouse)
from tests.test_gpu_ba_window import to_host

pytestmark = pytest.mark.gpu

SENT = -9
MAP_KEYS = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf", "obs_feat")


def padded(a, n, fill=SENT):
    fill = 77 if a.dtype == np.uint8 else fill
    out = np.full((n,) + a.shape[1:], fill, a.dtype)
    out[:len(a)] = a
    return out


def upload(torch, m, ba, ref_kf, NMPcap, OBScap):
    """the map in capacity buffers, sentinels behind the contents -> (map dict, ba dict, mp_ref_kf, sizes)"""
    NMP, NKF, NOBS = len(m["mp_valid"]), len(m["kf_valid"]), len(m["obs_kf"])
    mm = {k: np.asarray(v) for k, v in m.items()}
    for k in mm:
        if k in map_grow._PER_POINT:
            mm[k] = padded(mm[k], NMPcap)
    mm["obs_ptr"], mm["obs_kf"] = padded(mm["obs_ptr"], NMPcap + 1), padded(mm["obs_kf"], OBScap)
    bb = dict(ba, obs_feat=padded(ba["obs_feat"], OBScap), mp_assoc=padded(ba["mp_assoc"], NMPcap))
    rk = None if ref_kf is None else torch.from_numpy(padded(np.asarray(ref_kf, np.int32), NMPcap)).cuda()
    return to_dev(torch, mm), to_dev(torch, bb), rk, (NMP, NKF, NOBS)


def download(md, bd, rk, sizes, NMP0):
    """the device's arrays cut to sizes, the new rows' mp_pos / mp_assoc, and everything behind the contents"""
    NMP, NKF, NOBS = sizes
    h = lambda t: t.cpu().numpy()
    rows = dict(mp_valid=h(md["mp_valid"])[:NMP], kf_valid=h(md["kf_valid"])[:NKF], kf_mp=h(md["kf_mp"])[:NKF], obs_ptr=h(md["obs_ptr"])[:NMP + 1],
                obs_kf=h(md["obs_kf"])[:NOBS], obs_feat=h(bd["obs_feat"])[:NOBS])
    tails = dict(rows=np.concatenate([h(md["mp_valid"])[NMP:].astype(np.int32) - 77 + SENT, h(md["obs_ptr"])[NMP + 1:], h(bd["mp_assoc"])[NMP:]] +
                                     ([h(rk)[NMP:]] if rk is not None else [])), obs_kf=h(md["obs_kf"])[NOBS:], obs_feat=h(bd["obs_feat"])[NOBS:])
    if rk is not None:
        rows["mp_ref_kf"] = h(rk)[:NMP]
    rows.update(new_pos=h(md["mp_pos"])[NMP0:NMP], new_assoc=h(bd["mp_assoc"])[NMP0:NMP], old_pos=h(md["mp_pos"])[:NMP0], old_assoc=h(bd["mp_assoc"])[:NMP0])
    return rows, tails


def same(dev, ref, what, keys):
    for k in keys:
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, a.shape, b.shape, a.ravel()[:12], b.ravel()[:12])


def device_add(torch, ctx, m, ba, ref_kf, lists, caps=None, counts=False, already_cap=None, slack=5):
    """gl_map_add on a fresh upload -> (rows, result[6], the dict of map_add, the device buffers)"""
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    new_mp, att = lists.get("new_mp"), lists.get("attach")
    if caps is None:
        n_req = (0 if att is None else len(att)) + (0 if lists.get("walk_kf") is None else len(lists["walk_kf"])) * m["kf_mp"].shape[1]
        caps = (NMP + (0 if new_mp is None else len(new_mp["pos"])) + slack, NOBS + n_req + slack)
    md, bd, rk, sizes = upload(torch, m, ba, ref_kf, *caps)
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()
    pad = lambda a: np.concatenate([a, np.zeros((7,) + a.shape[1:], a.dtype)]) if counts else a  # (zeros behind a count: must not be read as entries)
    cnt = lambda a: torch.tensor([len(a)], dtype=torch.int32, device="cuda") if counts else None
    kw = {}
    if new_mp is not None:
        kw.update(new_mp={k: T(pad(np.asarray(v)), np.float64 if k == "pos" else np.int32) for k, v in new_mp.items()}, n_new_mp=cnt(new_mp["pos"]))
    if lists.get("new_kf") is not None:
        kw.update(new_kf=T(pad(np.asarray(lists["new_kf"], np.int32)), np.int32), n_new_kf=cnt(lists["new_kf"]))
    if att is not None:
        a = pad(np.asarray(att, np.int32).reshape(-1, 3))
        kw.update(attach=dict(mp=T(a[:, 0], np.int32), kf=T(a[:, 1], np.int32), feat=T(a[:, 2], np.int32)), n_attach=cnt(att))
    if lists.get("walk_kf") is not None:
        kw.update(walk_kf=T(pad(np.asarray(lists["walk_kf"], np.int32)), np.int32), n_walk=cnt(lists["walk_kf"]))
    def call(torch, ctx):
        r = map_grow.map_add(ctx, md, bd, sizes, mp_ref_kf=rk, want_new_pos=True, already_cap=already_cap, **kw)
        torch.cuda.synchronize()
        return r
    r = run(call, torch, ctx)
    rows, tails = download(md, bd, rk, r["sizes"], NMP)
    rows.update(obs_new_pos=r["obs_new_pos"].cpu().numpy(), already_mp=r["already_mp"].cpu().numpy())
    result = list(r["needed"][::2]) + [r["n_attached"], r["n_skipped"], r["n_already"], r["status"]]
    assert all((t == SENT).all() for t in tails.values()), "written behind the new sizes"
    assert r["map"]["obs_kf"].shape[0] == r["sizes"][2] and r["map"]["obs_ptr"].shape[0] == r["sizes"][0] + 1 and r["map"]["obs_kf"].data_ptr() == md["obs_kf"].data_ptr()
    return rows, result, r, (md, bd, rk)


ADD_KEYS = MAP_KEYS + ("mp_ref_kf", "obs_new_pos", "already_mp")


def check_add(dev, res_dev, ref, res_ref, m, ba, new_mp, what):
    assert res_dev == res_ref, (what, res_dev, res_ref)
    same(dev, ref, what, ADD_KEYS)
    if new_mp is not None:
        assert dev["new_pos"].tobytes() == np.asarray(new_mp["pos"], np.float64).tobytes() and np.array_equal(dev["new_assoc"], new_mp["assoc"]), what
    assert dev["old_pos"].tobytes() == np.asarray(m["mp_pos"]).tobytes() and np.array_equal(dev["old_assoc"], ba["mp_assoc"]), what


def device_fuse(torch, ctx, m, ba, kf, cand, best, OBScap=None, repl_cap=None):
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    md, bd, _, sizes = upload(torch, m, ba, None, NMP + 3, NOBS + len(cand) if OBScap is None else OBScap)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()
    def call(torch, ctx):
        r = map_grow.map_fuse(ctx, md, bd, kf, T(cand), T(best), sizes=sizes, repl_cap=repl_cap, want_new_pos=True)
        torch.cuda.synchronize()
        return r
    r = run(call, torch, ctx)
    rows, tails = download(md, bd, None, r["sizes"], NMP)
    rows.update(obs_new_pos=r["obs_new_pos"].cpu().numpy(), repl_src=r["repl_src"].cpu().numpy(), repl_tgt=r["repl_tgt"].cpu().numpy())
    n = r["sizes"][2]  # (the entries behind the new NOBS are not written: what they held, sentinels behind the old NOBS)
    assert (tails["rows"] == SENT).all() and np.array_equal(tails["obs_kf"], padded(m["obs_kf"], len(md["obs_kf"]))[n:]), "written behind the new sizes"
    assert np.array_equal(tails["obs_feat"], padded(ba["obs_feat"], len(md["obs_kf"]))[n:]), "written behind the new sizes"
    return rows, [r["needed"][2], r["n_fused"], r["n_attached"], r["n_replaced"], r["status"]], r, (md, bd)


FUSE_KEYS = MAP_KEYS + ("obs_new_pos", "repl_src", "repl_tgt")


# ---- the hand-built scenes

@pytest.mark.parametrize("name", list(GS.FUSE))
def test_map_fuse_hand_built(gpu, name):
    torch, ctx = gpu
    sc = GS.hand_scene(GS.FUSE, name)
    ref, res = G.map_fuse(sc["m"], sc["ba"], 0, sc["cand"], sc["best"])
    assert res == sc["out"]["result"]  # (the model gives the declared output: tests/test_map_grow_ref.py)
    dev, res_dev, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], 0, sc["cand"], sc["best"])
    assert res_dev == res, (name, res_dev, res)
    same(dev, ref, name, FUSE_KEYS)


def add_lists_of(sc):
    n = sc.get("new_mp", 0)
    return dict(new_mp=GS.new_points(n) if n else None, new_kf=sc.get("new_kf"), attach=sc.get("attach"), walk_kf=sc.get("walk"))


@pytest.mark.parametrize("counts", [False, True])
@pytest.mark.parametrize("name", list(GS.ADD))
def test_map_add_hand_built(gpu, name, counts):
    torch, ctx = gpu
    sc = GS.hand_scene(GS.ADD, name)
    ls = add_lists_of(sc)
    ref, res = G.map_add(sc["m"], sc["ba"], sc["mp_ref_kf"], ls["new_mp"], ls["new_kf"] or (), ls["attach"] or (), ls["walk_kf"] or ())
    assert res == sc["out"]["result"]
    dev, res_dev, _, _ = device_add(torch, ctx, sc["m"], sc["ba"], sc["mp_ref_kf"], ls, counts=counts)
    check_add(dev, res_dev, ref, res, sc["m"], sc["ba"], ls["new_mp"], (name, counts))


# ---- the random scenes, the large one

@pytest.mark.parametrize("name,seed", GS.RANDOM_FUSE + (GS.BIG_FUSE,))
def test_map_fuse_random(gpu, name, seed):
    """colliding candidate lists (every branch: tests/test_map_grow_ref.py); `euroc`: 180 000 points, the rebuild's scan crosses 44 tiles"""
    torch, ctx = gpu
    sc = ES.scene(name, name in ES.CLAMP)
    kf, cand, best = GS.fuse_lists(sc, seed)
    ref, res = G.map_fuse(sc["m"], sc["ba"], kf, cand, best)
    assert res[3] >= 3 and res[2] >= 1
    dev, res_dev, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best)
    assert res_dev == res, (name, res_dev, res)
    same(dev, ref, name, FUSE_KEYS)


@pytest.mark.parametrize("name,seed", GS.RANDOM_ADD + (GS.BIG_ADD,))
def test_map_add_random(gpu, name, seed):
    torch, ctx = gpu
    m, ba, ref_kf, ls = GS.add_lists(ES.scene(name, name in ES.CLAMP), seed)
    ref, res = G.map_add(m, ba, ref_kf, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"])
    assert res[2] > 20 and res[3] >= 6 and res[4] >= 1
    dev, res_dev, _, _ = device_add(torch, ctx, m, ba, ref_kf, ls, counts=name == "small")
    check_add(dev, res_dev, ref, res, m, ba, ls["new_mp"], name)


# ---- capacities, nothing, determinism

def test_one_short_of_a_capacity_writes_nothing(gpu):
    """exactly enough: the model; one short of NMPcap, of OBScap, of both: the map's bytes unchanged, the needed sizes and the bit
    returned; the same call with room afterwards equals the model.  gl_map_fuse: OBScap = NOBS + n_cand and one below"""
    torch, ctx = gpu
    m, ba, ref_kf, ls = GS.add_lists(ES.scene("tiny"), 1)
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    ref, res = G.map_add(m, ba, ref_kf, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"])
    need_mp, need_obs = res[0], res[1]
    assert need_mp > NMP and need_obs > NOBS
    for caps, bits in (((need_mp, need_obs), 0), ((need_mp - 1, need_obs), G.MP_TRUNCATED), ((need_mp, need_obs - 1), G.OBS_TRUNCATED),
                       ((need_mp - 1, need_obs - 1), G.MP_TRUNCATED | G.OBS_TRUNCATED)):
        dev, res_dev, r, (md, bd, rk) = device_add(torch, ctx, m, ba, ref_kf, ls, caps=caps)
        assert res_dev == res[:5] + [bits], (caps, res_dev)
        if not bits:
            check_add(dev, res_dev, ref, res, m, ba, ls["new_mp"], caps)
            continue
        assert r["sizes"] == (NMP, len(m["kf_valid"]), NOBS)
        for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf"):
            assert dev[k].tobytes() == np.asarray(m[k]).tobytes(), (caps, k)
        assert dev["obs_feat"].tobytes() == ba["obs_feat"].tobytes() and dev["mp_ref_kf"].tobytes() == ref_kf.tobytes()
        assert np.array_equal(dev["already_mp"], ref["already_mp"])
    sc = ES.scene("tiny")
    kf, cand, best = GS.fuse_lists(sc, 2)
    ref, res = G.map_fuse(sc["m"], sc["ba"], kf, cand, best)
    NOBS = len(sc["m"]["obs_kf"])
    dev, res_dev, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best, OBScap=NOBS + len(cand))
    assert res_dev == res
    same(dev, ref, "fuse, exactly enough", FUSE_KEYS)
    dev, res_dev, r, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best, OBScap=NOBS + len(cand) - 1)
    assert res_dev == [NOBS + len(cand), 0, 0, 0, G.OBS_TRUNCATED] and r["sizes"][2] == NOBS
    for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf"):
        assert dev[k].tobytes() == np.asarray(sc["m"][k]).tobytes(), k
    assert dev["obs_feat"].tobytes() == sc["ba"]["obs_feat"].tobytes()


def test_list_capacities_keep_the_true_counts(gpu):
    """already_cap / repl_cap below the counts: the first entries, the true count, the bit - and the MAP edit is complete"""
    torch, ctx = gpu
    m, ba, ref_kf, ls = GS.add_lists(ES.scene("tiny"), 1)
    ref, res = G.map_add(m, ba, ref_kf, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"], already_cap=1)
    assert res[4] > 1 and res[5] == G.ALREADY_TRUNCATED
    dev, res_dev, _, _ = device_add(torch, ctx, m, ba, ref_kf, ls, already_cap=1)
    check_add(dev, res_dev, ref, res, m, ba, ls["new_mp"], "already_cap")
    sc = ES.scene("tiny")
    kf, cand, best = GS.fuse_lists(sc, 2)
    ref, res = G.map_fuse(sc["m"], sc["ba"], kf, cand, best, repl_cap=2)
    assert res[3] > 2 and res[4] == G.REPL_TRUNCATED
    dev, res_dev, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best, repl_cap=2)
    assert res_dev == res
    same(dev, ref, "repl_cap", FUSE_KEYS)


def test_nothing_in_any_list_changes_nothing(gpu):
    torch, ctx = gpu
    sc = ES.scene("small")
    m, ba = sc["m"], sc["ba"]
    none = np.zeros(0, np.int32)
    for ls in (dict(), dict(new_mp=GS.new_points(0), new_kf=none, attach=none.reshape(0, 3), walk_kf=none)):
        dev, res, _, _ = device_add(torch, ctx, m, ba, sc["mp_ref_kf"], ls)
        assert res == [len(m["mp_valid"]), len(m["obs_kf"]), 0, 0, 0, 0]
        for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf"):
            assert dev[k].tobytes() == np.asarray(m[k]).tobytes(), k
        assert dev["obs_feat"].tobytes() == ba["obs_feat"].tobytes() and np.array_equal(dev["obs_new_pos"], np.arange(len(m["obs_kf"])))
    for cand, best in ((none, none), (np.array([5, 6], np.int32), np.array([-1, -1], np.int32))):
        dev, res, _, _ = device_fuse(torch, ctx, m, ba, int(sc["rows"][0]), cand, best)
        assert res == [len(m["obs_kf"]), 0, 0, 0, 0]
        for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf"):
            assert dev[k].tobytes() == np.asarray(m[k]).tobytes(), k
        assert dev["obs_feat"].tobytes() == ba["obs_feat"].tobytes() and np.array_equal(dev["obs_new_pos"], np.arange(len(m["obs_kf"])))


def test_twenty_runs_give_the_same_bytes(gpu):
    """integer stores and integer atomics on words the inputs determine: the same two calls 20 times, each on a fresh upload"""
    torch, ctx = gpu
    (an, aseed), (fn, fseed) = GS.RANDOM_ADD[1], GS.RANDOM_FUSE[1]  # (lists whose branch coverage tests/test_map_grow_ref.py asserts)
    m, ba, ref_kf, ls = GS.add_lists(ES.scene(an, an in ES.CLAMP), aseed)
    sc = ES.scene(fn, fn in ES.CLAMP)
    kf, cand, best = GS.fuse_lists(sc, fseed)
    first = None
    for _ in range(20):
        a, ra, _, _ = device_add(torch, ctx, m, ba, ref_kf, ls)
        f, rf, _, _ = device_fuse(torch, ctx, sc["m"], sc["ba"], kf, cand, best)
        got = b"".join(np.asarray(a[k]).tobytes() for k in ADD_KEYS) + b"".join(np.asarray(f[k]).tobytes() for k in FUSE_KEYS) + bytes(str((ra, rf)), "ascii")
        first = got if first is None else first
        assert got == first


# ---- the readers on the grown map, the round trip

def grown(torch, ctx, name="small"):
    """a device add + fuse and the model's -> (device map / ba dicts cut to the sizes, mp_ref_kf; the model's rows as m2, ba2, ref_kf2)"""
    sc = ES.scene(name, name in ES.CLAMP)
    g = GS.grown_lists(name)  # (its fuse list exercises every branch: asserted in tests/test_map_grow_ref.py)
    m, ba, ref_kf, ls, rows1, res1, m1, ba1, kf, cand, best = (g[k] for k in ("m", "ba", "ref_kf", "lists", "rows1", "res1", "m1", "ba1", "kf", "cand", "best"))
    rows2, res2 = G.map_fuse(m1, ba1, kf, cand, best)
    assert res1[2] > 20 and res2[3] >= 3
    m2, ba2 = G.apply_rows(m1, ba1, rows2)
    _, _, r, (md, bd, rk) = device_add(torch, ctx, m, ba, ref_kf, ls, slack=len(cand))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r2 = map_grow.map_fuse(ctx, md, bd, kf, T(cand), T(best), sizes=r["sizes"])
    assert r2["sizes"] == (len(m2["mp_valid"]), len(m2["kf_valid"]), len(m2["obs_kf"])) and r2["status"] == 0
    return r2["map"], r2["ba"], rk[:r2["sizes"][0]], m2, ba2, rows1["mp_ref_kf"], sc["rows"]


def test_the_readers_take_the_grown_map(gpu):
    """gl_update_connections, gl_ba_window_build, gl_update_local_map and gl_map_remove on the device-grown arrays (views cut to the new
    sizes) give bit for bit what they give on the model's rows uploaded afresh"""
    torch, ctx = gpu
    mm, bb, rk, m2, ba2, ref2, rows = grown(torch, ctx)
    for k in MAP_KEYS[:5]:
        assert mm[k].cpu().numpy().tobytes() == np.asarray(m2[k]).tobytes(), k
    fresh_m, fresh_b = to_dev(torch, m2), to_dev(torch, ba2)
    rw = torch.from_numpy(rows).cuda()
    sc2 = dict(m=m2, ba=ba2)
    rm_mp, erase, rm_kf = ES.removals(sc2, 3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = []
    for m_, b_, rk_ in ((mm, bb, rk.contiguous()), (fresh_m, fresh_b, T(ref2))):
        conn = api.update_connections(ctx, m_, rw, Ccap=64, want_count=True)
        _, wins = R.ba_window_build(m2, ba2, rows, S.empty_slab(len(rows), (1, 1, 1, 1)))
        slab = to_dev(torch, S.empty_slab(len(rows), S.caps_of(wins)))
        api.ba_window_build(ctx, m_, b_, rw, slab)
        feat = m_["kf_mp"][rw.long()].clone()
        lists = api.local_map_lists(len(rows), 128, 4096, len(m2["kf_valid"]), device="cuda")
        api.update_local_map(ctx, {k: m_[k] for k in ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp")}, feat, lists)
        torch.cuda.synchronize()
        out = dict(conn=to_host(conn), slab=to_host(slab), feat=dict(feat=feat.cpu().numpy()), lists=to_host(lists))
        e = api.map_remove(ctx, m_, b_, erase_obs=T(erase), rm_kf=T(rm_kf), rm_mp=T(rm_mp), mp_ref_kf=rk_, want_new_pos=True)  # (last: it edits)
        n = e["nobs"]
        out["removed"] = dict({k: m_[k].cpu().numpy() for k in MAP_KEYS[:4]}, obs_kf=m_["obs_kf"].cpu().numpy()[:n], obs_feat=b_["obs_feat"].cpu().numpy()[:n],
                              ref=rk_.cpu().numpy(), dead=e["dead_mp"].cpu().numpy(), new_pos=e["obs_new_pos"].cpu().numpy())
        outs.append(out)
    a, b = outs
    for grp in b:
        same(a[grp], b[grp], grp, list(b[grp]))
    # (the colliding triples leave slots that another point's entry still names: there gl_map_remove clears a slot only if it holds the
    # point, the model of map_edit_ref clears it always - so the removal is held to the fresh upload, not to that model)
    ref, _ = E.map_remove(m2, ba2, rm_mp, erase, rm_kf, ref2)
    assert len(ref["dead_mp"]) > 0 and len(ref["obs_kf"]) < len(m2["obs_kf"])


def test_add_then_remove_gives_the_entries_back(gpu):
    """map_add of a key-frame (new_kf + walk), then map_remove(rm_kf = [it]): the model says which points survive the removal, and for
    those the entry arrays are what they were before the add"""
    torch, ctx = gpu
    m, ba, ref_kf, ls = GS.add_lists(ES.scene("small", True), 2)
    kf = int(ls["new_kf"][0])
    ls = dict(new_kf=np.array([kf], np.int32), walk_kf=np.array([kf], np.int32))
    rows1, res1 = G.map_add(m, ba, ref_kf, None, ls["new_kf"], (), ls["walk_kf"])
    assert res1[2] > 5
    m1, ba1 = G.apply_rows(m, ba, rows1)
    rows2, _ = E.map_remove(m1, ba1, rm_kf=[kf], mp_ref_kf=rows1["mp_ref_kf"])
    _, _, r, (md, bd, rk) = device_add(torch, ctx, m, ba, ref_kf, ls)
    e = api.map_remove(ctx, r["map"], r["ba"], rm_kf=torch.tensor([kf], dtype=torch.int32, device="cuda"), mp_ref_kf=rk[:r["sizes"][0]].contiguous())
    n = e["nobs"]
    got = dict({k: r["map"][k].cpu().numpy() for k in MAP_KEYS[:4]}, obs_kf=md["obs_kf"].cpu().numpy()[:n], obs_feat=bd["obs_feat"].cpu().numpy()[:n])
    same(got, rows2, "add then remove", MAP_KEYS)
    held = np.zeros(len(m["mp_valid"]), bool)  # the points that observed the key-frame before the add lose that entry with it
    held[np.repeat(np.arange(len(held)), np.diff(m["obs_ptr"]))[m["obs_kf"] == kf]] = True
    alive = (rows2["mp_valid"] != 0) & ~held
    cnt0, cnt2 = np.diff(m["obs_ptr"]), np.diff(rows2["obs_ptr"])
    assert alive.sum() > 100 and np.array_equal(cnt0[alive], cnt2[alive])  # the other survivors hold what they held before the add
    for p in np.nonzero(alive)[0][:200]:
        assert np.array_equal(got["obs_kf"][rows2["obs_ptr"][p]:rows2["obs_ptr"][p + 1]], m["obs_kf"][m["obs_ptr"][p]:m["obs_ptr"][p + 1]])


# ---- arguments

def test_arguments(gpu):
    """a stale or wrong buffer raises in the wrapper; the library refuses bad arguments with GL_ERR_ARG and launches nothing"""
    torch, ctx = gpu
    sc = ES.scene("tiny")
    m, ba = sc["m"], sc["ba"]
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    md, bd, rk, sizes = upload(torch, m, ba, sc["mp_ref_kf"], NMP + 4, NOBS + 8)
    z = lambda *sh: torch.zeros(sh, dtype=torch.int32, device="cuda")
    before = {k: v.clone() for k, v in md.items()}
    for kw, msg in ((dict(sizes=(NMP + 5, sizes[1], NOBS)), "outside the buffers"), (dict(sizes=(NMP, sizes[1], NOBS + 9)), "outside the buffers"),
                    (dict(new_kf=z(1).long()), "int32"), (dict(attach=dict(mp=z(2), kf=z(2), feat=z(3))), "shape"),
                    (dict(new_mp=dict(pos=torch.zeros(2, 3, device="cuda"), assoc=z(2), ref_kf=z(2))), "float64"),
                    (dict(new_mp=dict(pos=torch.zeros(2, 3, dtype=torch.float64, device="cuda"), assoc=z(2))), "missing"),
                    (dict(walk_kf=z(4)[::2]), "contiguous"), (dict(mp_ref_kf=rk[:NMP].contiguous()), "shape")):
        with pytest.raises(AssertionError, match=msg):
            map_grow.map_add(ctx, md, bd, **dict(dict(sizes=sizes, mp_ref_kf=rk), **kw))
    with pytest.raises(AssertionError, match="shape"):
        map_grow.map_add(ctx, md, dict(bd, obs_feat=bd["obs_feat"][:NOBS].contiguous()), sizes)  # a stale buffer: shorter than obs_kf
    with pytest.raises(AssertionError, match="outside"):
        map_grow.map_fuse(ctx, md, bd, sizes[1], z(1), z(1), sizes=sizes)
    with pytest.raises(AssertionError, match="shape"):
        map_grow.map_fuse(ctx, md, bd, 0, z(2), z(3), sizes=sizes)
    ed = api._map_edit(md, bd, None, NMP + 4, md["obs_ptr"].device)
    ls, o = map_grow._lib.gl_map_add_lists(), map_grow._lib.gl_map_add_out()
    res = z(6)
    o.result = api._ptr(res)
    lib = ctx.lib
    assert lib.gl_map_add(ctx.h, NMP, sizes[1], 24, NOBS, NMP - 1, NOBS, C.byref(ed), None, None, C.byref(ls), C.byref(o)) == -1
    assert lib.gl_last_error_string().decode().endswith("a capacity below the size")
    assert lib.gl_map_add(ctx.h, NMP, sizes[1], 24, NOBS, NMP, NOBS, None, None, None, None, None) == -1
    assert lib.gl_last_error_string().decode().endswith("null argument")
    ls.attach_cap, ls.att_mp = 2, api._ptr(z(2))
    assert lib.gl_map_add(ctx.h, NMP, sizes[1], 24, NOBS, NMP, NOBS, C.byref(ed), None, None, C.byref(ls), C.byref(o)) == -1
    assert lib.gl_last_error_string().decode().endswith("null att_kf / att_feat")
    fo = map_grow._lib.gl_map_fuse_out()
    fo.result = api._ptr(res)
    uvr = api._ptr(bd["kf_uvr"])
    assert lib.gl_map_fuse(ctx.h, NMP, sizes[1], 24, NOBS, NOBS, C.byref(ed), uvr, sizes[1], 0, None, None, C.byref(fo)) == -1
    assert lib.gl_last_error_string().decode().endswith("kf outside the table")
    assert lib.gl_map_fuse(ctx.h, NMP, sizes[1], 24, NOBS, NOBS, C.byref(ed), uvr, 0, 1, None, None, C.byref(fo)) == -1
    assert lib.gl_last_error_string().decode().endswith("null cand_mp / best_idx")
    fo.repl_cap = 4
    assert lib.gl_map_fuse(ctx.h, NMP, sizes[1], 24, NOBS, NOBS, C.byref(ed), uvr, 0, 0, None, None, C.byref(fo)) == -1
    assert lib.gl_last_error_string().decode().endswith("null repl_src / repl_tgt")
    torch.cuda.synchronize()
    assert all(bool((md[k] == before[k]).all()) for k in before) and bool((res == 0).all())


# ---- one composed mapping pass

POINT_OUT = (("mp_desc", np.uint8, (32,)), ("mp_normal", np.float64, (3,)), ("mp_max_dist", np.float32, ()), ("mp_min_dist", np.float32, ()))


def pass_inputs(sc, n_new=3):
    """the geometric scene with its key-frame handed over NEW (kf_mp row filled, nothing observes it, invalid) and the additions of the
    pass: the walk, n_new new points with two triples each -> (m0, ba0, ref0, lists, targets)"""
    K = sc["kf_row"]
    m0, ba0 = GS.strip_key_frame(sc["m"], sc["ba"], K)
    NMP = len(m0["mp_valid"])
    t0 = GS.GEO_TARGETS[0]
    free_k, free_t = np.nonzero(m0["kf_mp"][K] < 0)[0], np.nonzero(m0["kf_mp"][t0] < 0)[0]
    n_new = min(n_new, len(free_k), len(free_t))
    assert n_new >= 2
    held = m0["kf_mp"][K][m0["kf_mp"][K] >= 0][:n_new]
    new = dict(pos=m0["mp_pos"][held] + 0.05, assoc=np.full(n_new, -1, np.int32), ref_kf=np.full(n_new, K, np.int32))
    att = np.array([t for i in range(n_new) for t in ((NMP + i, K, free_k[i]), (NMP + i, t0, free_t[i]))], np.int32)
    return m0, ba0, sc["mp_ref_kf"], dict(new_mp=new, new_kf=np.array([K], np.int32), attach=att, walk_kf=np.array([K], np.int32)), GS.GEO_TARGETS


def refresh(ctx, md, bd, rk, kf_desc, sizes):
    """gl_update_map_points (descriptor, normal, distances) of every point on the arrays cut to sizes"""
    mm, bb = map_grow.map_views(md, bd, sizes)
    NMP = sizes[0]
    api.update_map_points(ctx, dict(twc=bb["kf_twc"], valid=mm["kf_valid"], oct=bb["kf_oct"], desc=kf_desc),
                          dict(pos=mm["mp_pos"], valid=mm["mp_valid"], ref_kf=rk[:NMP], obs_ptr=mm["obs_ptr"], obs_kf=mm["obs_kf"], obs_feat=bb["obs_feat"]),
                          dict(desc=mm["mp_desc"], normal=mm["mp_normal"], max_dist=mm["mp_max_dist"], min_dist=mm["mp_min_dist"]))


def with_point_arrays(m, NMPcap=None):
    n = len(m["mp_valid"]) if NMPcap is None else NMPcap
    return dict(m, **{k: np.full((n,) + sh, 0xA5 if dt == np.uint8 else -7, dt) for k, dt, sh in POINT_OUT})


def device_pass(torch, ctx, sc, cam, cands):
    """the pass on the resident arrays -> (sizes, the arrays cut to them, the per-step results)"""
    m0, ba0, ref0, ls, targets = pass_inputs(sc)
    NMP, NOBS = len(m0["mp_valid"]), len(m0["obs_kf"])
    NMPcap, OBScap = NMP + 16, NOBS + 140 + 16 + len(targets) * 140
    md, bd, rk, sizes = upload(torch, with_point_arrays(m0), ba0, ref0, NMPcap, OBScap)
    T = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()
    kf_desc = T(sc["kf_desc"], np.uint8)
    new, att = ls["new_mp"], ls["attach"]
    a = map_grow.map_add(ctx, md, bd, sizes, new_mp=dict(pos=T(new["pos"], np.float64), assoc=T(new["assoc"]), ref_kf=T(new["ref_kf"])), new_kf=T(ls["new_kf"]),
                         attach=dict(mp=T(att[:, 0]), kf=T(att[:, 1]), feat=T(att[:, 2])), walk_kf=T(ls["walk_kf"]), mp_ref_kf=rk)
    assert a["status"] == 0
    sizes = a["sizes"]
    steps = [[a["n_attached"], a["n_skipped"], a["n_already"]]]
    refresh(ctx, md, bd, rk, kf_desc, sizes)
    for t, cand in zip(targets, cands):
        r = map_grow.fuse_observations_from_map(ctx, cam, md, bd, dict(desc=kf_desc), t, T(cand), sizes=sizes)
        assert r["status"] == 0
        sizes = r["sizes"]
        steps.append([r["n_fused"], r["n_attached"], r["n_replaced"]] + r["repl_src"].tolist() + r["repl_tgt"].tolist() + r["best_idx"].tolist())
        refresh(ctx, md, bd, rk, kf_desc, sizes)
    torch.cuda.synchronize()
    mm, bb = map_grow.map_views(md, bd, sizes)
    out = {k: mm[k].cpu().numpy() for k in MAP_KEYS[:5] + tuple(k for k, _, _ in POINT_OUT) + ("mp_pos",)}
    out.update(obs_feat=bb["obs_feat"].cpu().numpy(), mp_assoc=bb["mp_assoc"].cpu().numpy(), mp_ref_kf=rk[:sizes[0]].cpu().numpy())
    return sizes, out, steps


def host_pass(torch, ctx, sc, cam):
    """the same pass with every edit made by the model on the host and the map uploaded afresh for each search
    -> (the model's final rows + the per-point arrays of the last refresh, the per-step results, the candidate lists)"""
    m, ba, ref, ls, targets = pass_inputs(sc)
    K = sc["kf_row"]
    T = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()
    kf_desc = T(sc["kf_desc"], np.uint8)
    rows, res = G.map_add(m, ba, ref, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"])
    steps = [res[2:5]]
    m, ba = G.apply_rows(m, ba, rows, dict(mp_pos=ls["new_mp"]["pos"]))
    ba["mp_assoc"] = np.concatenate([ba["mp_assoc"], ls["new_mp"]["assoc"]])
    ref = rows["mp_ref_kf"]
    cands, point_out = [], None
    for t in targets:
        cand = m["kf_mp"][K][m["kf_mp"][K] >= 0].astype(np.int32)  # curr_kf_->getMapPoints() as the map holds them now
        cands.append(cand)
        md, bd, rk, sizes = upload(torch, with_point_arrays(m), ba, ref, len(m["mp_valid"]), len(m["obs_kf"]) + len(cand))
        refresh(ctx, md, bd, rk, kf_desc, sizes)
        best = map_grow.fuse_observations_from_map(ctx, cam, md, bd, dict(desc=kf_desc), t, T(cand), sizes=sizes)["best_idx"].cpu().numpy()
        rows, res = G.map_fuse(m, ba, t, cand, best)
        steps.append(res[1:4] + rows["repl_src"].tolist() + rows["repl_tgt"].tolist() + best.tolist())
        m, ba = G.apply_rows(m, ba, rows)
    md, bd, rk, sizes = upload(torch, with_point_arrays(m), ba, ref, len(m["mp_valid"]), len(m["obs_kf"]))
    refresh(ctx, md, bd, rk, kf_desc, sizes)
    torch.cuda.synchronize()
    out = dict({k: np.asarray(m[k]) for k in MAP_KEYS[:5] + ("mp_pos",)}, obs_feat=ba["obs_feat"], mp_assoc=ba["mp_assoc"], mp_ref_kf=ref)
    out.update({k: md[k].cpu().numpy() for k, _, _ in POINT_OUT})
    return out, steps, cands


def test_composed_pass_equals_the_models_edits_uploaded(gpu, map_v1, gt_sync):
    """a key-frame's additions on the geometric scene with nothing re-uploaded - new key-frame rows, the walk, new points with two triples
    each, fuse_observations_from_map into three target key-frames with update_map_points between them - against the same pass with
    every edit made by the model on the host and the whole map uploaded afresh before each search: every map array, the per-point
    arrays of the last refresh, the counts, the replacement lists and best_idx of every step"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam = api.Camera()
    sc = GS.geo_scene(mean, cov, gt_sync["V1_01_easy"])
    want, steps_h, cands = host_pass(torch, ctx, sc, cam)
    fused = np.array([s[:3] for s in steps_h[1:]])
    print("pass: add", steps_h[0], "fuse (fused, attached, replaced) per target", fused.tolist())
    assert steps_h[0][0] > 100 and fused[:, 1].sum() >= 1 and fused[:, 2].sum() >= 1  # the walk attached; the fuse attached and replaced
    sizes, got, steps_d = device_pass(torch, ctx, sc, cam, cands)
    assert steps_d == steps_h
    assert sizes == (len(want["mp_valid"]), len(want["kf_valid"]), len(want["obs_kf"]))
    alive = want["mp_valid"] != 0  # (update_map_points leaves the rows of an invalid point as they are)
    for k, _, _ in POINT_OUT:
        got[k], want[k] = got[k][alive], want[k][alive]
    same(got, want, "pass", list(want))
