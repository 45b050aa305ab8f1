"""gl_covis_update, gl_covis_remove, gl_covis_best, gl_fuse_targets, gl_fuse_candidates and covis.search_in_neighbors_from_map against
tests/covis_ref.py - integers only, so every array is compared exactly, guard words stand behind every array a call may write, and the
expected output always comes from the model, never from the device: random edit sequences (exact after every step), rows at the
lengths where the kernels change chunk (a wave, a workgroup), the capacity rule, conn_* against gl_update_connections bit for bit,
the candidate list at the edges of a wave, a workgroup and a scan tile, and the composite against the split route it replaces."""
import copy

import numpy as np
import pytest

from gmmloc_amd import api, covis, frame_step, map_grow, map_stats
from tests import covis_cases as CC
from tests import covis_dev as D
from tests import covis_ref as R
from tests import map_grow_scenes as GS
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse)
from tests.test_covis_ref import apply_step
from tests.test_gpu_map_grow import refresh, upload, with_point_arrays

pytestmark = pytest.mark.gpu


def same_graph(got, want, what):
    for k in D.GRAPH_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def same_out(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def test_random_edit_sequence(gpu):
    """250 edits on 40 key-frames of 32 slots, about 600 points: the device's graph equals the numpy rows after EVERY step, word for word
    over the whole tables (what a call leaves behind a row's end included), and the object model on every row's contents"""
    torch, ctx = gpu
    m = CC.random_map(11)
    W = CC.R_NKF
    md, g = R.Model(CC.R_NKF), CC.graph(CC.R_NKF, W, {})
    dg = D.DevGraph(torch, copy.deepcopy(g))
    mdev = D.dev_map(torch, m)
    n_changed = n_removed = 0
    for i, step in enumerate(CC.random_steps(111, 250)):
        want = apply_step(step, m, md, g)
        if step[0] == "flip":
            mdev = D.dev_map(torch, m)
            continue
        if step[0] == "update":
            same_out(D.d_update(torch, ctx, mdev, dg, step[1], 64), want, (i, step))
            n_changed += int(want["result"][2])
        else:
            assert np.array_equal(D.d_remove(torch, ctx, dg, CC.R_NKF, step[1], step[2]), want), (i, step)
            n_removed += int(want[0])
        same_graph(dg.host(), g, (i, step))
        ref = md.rows(W)
        assert all(np.array_equal(ref[k], g[k]) for k in ("cov_n", "cov_nord", "best_cov")), (i, step)
        if i % 25 == 0:
            kf = int(np.argmax(g["cov_nord"]))
            same_out(D.d_targets(torch, ctx, dg, CC.R_NKF, m["kf_valid"], kf, 10, 5, 60), R.rows_targets(g, CC.R_NKF, m["kf_valid"], kf, 10, 5, 60), (i, "targets", kf))
    assert n_changed > 50 and n_removed > 20, (n_changed, n_removed)


def _long_row(L, where):
    """key-frame 1 names the rows 2 .. L + 1; key-frame 0 shares w points with it so that its entry lands in front, in the middle (among
    ties) or at the end"""
    i = np.arange(L)
    if where == "front":
        w, ws = 40, 39 - (i * 39) // L
    elif where == "end":
        w, ws = 16, 17 + ((L - 1 - i) * 20) // L
    else:
        w, ws = 30, 40 - (i * 20) // L
    rows = {1: (list(zip((i + 2).tolist(), ws.tolist())), min(3, L))}
    return w, rows


@pytest.mark.parametrize("where", ["front", "middle", "end"])
@pytest.mark.parametrize("L", [63, 64, 65, 255, 256, 257])
def test_insertion_into_a_long_row(gpu, L, where):
    torch, ctx = gpu
    w, rows = _long_row(L, where)
    nkf = L + 3
    m = CC.shared_map({(0, 1): w}, nkf=nkf)
    g = CC.graph(nkf, L + 1, rows)
    dg = D.DevGraph(torch, copy.deepcopy(g))
    want = R.rows_update(g, m, 0, 4)
    at = int(np.flatnonzero(g["cov_kf"][1] == 0)[0])
    assert int(g["cov_n"][1]) == L + 1 and {"front": at == 0, "end": at == L, "middle": 0 < at < L}[where], (at, L)
    same_out(D.d_update(torch, ctx, D.dev_map(torch, m), dg, 0, 4), want, (L, where))
    same_graph(dg.host(), g, (L, where))
    # ... and out of it again: the removal of key-frame 0 shifts the row back
    res = R.rows_remove(g, nkf, [0], -1)
    assert np.array_equal(D.d_remove(torch, ctx, dg, nkf, [0], -1), res) and res.tolist() == [1, 0, 1, 0]
    same_graph(dg.host(), g, (L, where, "removed"))


def test_capacity_at_the_need_and_one_below(gpu):
    """the own row needs five entries: Wcap = 5 takes it, Wcap = 4 refuses - every byte of the tables as it was, the width reported"""
    torch, ctx = gpu
    m = CC.shared_map({(0, k): k + 1 for k in range(1, 6)})
    for W, ok in ((5, True), (4, False)):
        g = CC.graph(CC.NKF, W, {2: ([(0, 99)], 1)})
        g0 = copy.deepcopy(g)
        dg = D.DevGraph(torch, copy.deepcopy(g))
        want = R.rows_update(g, m, 0, 8)
        out = D.d_update(torch, ctx, D.dev_map(torch, m), dg, 0, 8)
        same_out(out, want, W)
        assert out["result"].tolist() == ([5, 0, 1, 0] if ok else [5, R.W_TRUNCATED, 0, 0])
        same_graph(dg.host(), g if ok else g0, W)


def test_grow_tables_after_a_refusal(gpu):
    torch, ctx = gpu
    m = CC.shared_map({(0, k): k + 1 for k in range(1, 6)})
    cov = covis.covis_alloc(CC.NKF, 2)
    out, cov2 = covis.update_connections_in_map(ctx, D.dev_map(torch, m), cov, 0)
    assert cov2["cov_kf"].shape == (CC.NKF, 5) and out["result"].tolist() == [5, 0, 1, 0]
    assert cov2["cov_kf"][0].tolist() == [5, 4, 3, 2, 1] and cov2["cov_n"].tolist() == [5, 0, 0, 0, 0, 1, 0]


def test_conn_equals_update_connections(gpu):
    """conn_kf / conn_w / n_conn and the GL_CONN_* bits: what gl_update_connections writes for the same row, bit for bit"""
    torch, ctx = gpu
    m = CC.random_map(12)
    mdev = D.dev_map(torch, m)
    n_trunc = 0
    for Ccap in (1, 2, 64):
        dg = D.DevGraph(torch, CC.graph(CC.R_NKF, CC.R_NKF, {}))
        for kf in range(CC.R_NKF):
            ref = api.update_connections(ctx, mdev, torch.tensor([kf], dtype=torch.int32, device="cuda"), Ccap=Ccap)
            out = D.d_update(torch, ctx, mdev, dg, kf, Ccap)
            n = int(ref["n_conn"][0])
            k = min(n, Ccap)
            assert out["n_conn"].tolist() == [n] and (out["result"][1] & 7) == int(ref["status"][0]), (Ccap, kf)
            assert np.array_equal(out["conn_kf"][:k], ref["conn_kf"][0, :k].cpu().numpy()) and np.array_equal(out["conn_w"][:k], ref["conn_w"][0, :k].cpu().numpy())
            n_trunc += n > Ccap
    assert n_trunc > 5


def test_best_below_at_and_above_the_prefix(gpu):
    torch, ctx = gpu
    m = CC.random_map(13)
    g = CC.graph(CC.R_NKF, CC.R_NKF, {})
    for step in CC.random_steps(113, 120):  # (the numpy rows make the graph: prefixes shorter than their rows and whole rows)
        apply_step(step, m, None, g)
    dg = D.DevGraph(torch, copy.deepcopy(g))
    nord = int(g["cov_nord"].max())
    assert nord >= 3 and (g["cov_nord"] < g["cov_n"]).any() and ((g["cov_nord"] == g["cov_n"]) & (g["cov_n"] > 1)).any()
    rows = list(range(CC.R_NKF)) + [-1, CC.R_NKF]
    for N in (nord - 1, nord, nord + 1, 0, 1):
        for Ccap in (nord, 2):
            same_out(D.d_best(torch, ctx, dg, CC.R_NKF, rows, N, Ccap), R.rows_best(g, CC.R_NKF, rows, N, Ccap), (N, Ccap))


def cand_inputs(npos):
    """6 000 key-frames of ONE slot over 3 000 points (a fifth invalid, some slots null or outside the table), npos targets, two of them
    outside the table"""
    rng = np.random.default_rng(npos)
    nkf, nmp = 6000, 3000
    m = dict(kf_mp=rng.integers(-1, nmp + 2, (nkf, 1)).astype(np.int32), mp_valid=(rng.random(nmp) < 0.8).astype(np.uint8),
             obs_ptr=np.zeros(nmp + 1, np.int32), obs_kf=np.zeros(0, np.int32), kf_valid=np.ones(nkf, np.uint8))
    tgt = rng.integers(0, nkf, npos).astype(np.int32)
    tgt[rng.integers(0, npos, 2)] = nkf + 1
    return m, tgt


@pytest.mark.parametrize("npos", [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_candidates_at_the_edges(gpu, npos):
    """one slot per key-frame, npos targets: the position grid ends one short of, at and one past a wave, a workgroup and a scan tile;
    the points repeat, so first occurrences are decided across chunks"""
    torch, ctx = gpu
    m, tgt = cand_inputs(npos)
    mdev = D.dev_map(torch, m)
    full = R.rows_candidates(m, tgt, npos, 3, npos)
    n = int(full["n_cand"][0])
    assert 0 < n < npos
    same_out(D.d_candidates(torch, ctx, mdev, tgt, npos, 3, npos), full, npos)
    same_out(D.d_candidates(torch, ctx, mdev, tgt, npos, 3, n - 1), R.rows_candidates(m, tgt, npos, 3, n - 1), (npos, "one below"))
    same_out(D.d_candidates(torch, ctx, mdev, tgt, npos - 1, 3, n), R.rows_candidates(m, tgt, npos - 1, 3, n), (npos, "count on the device"))


# ---- the composite
POINT_KEYS = ("mp_desc", "mp_normal", "mp_max_dist", "mp_min_dist")


def _scene(torch, ctx, sc, invalid=()):
    """the geometric scene in capacity buffers with every point refreshed, the graph built by gl_covis_update over its key-frames in row
    order, counters and mp_replaced -> a dict of device state"""
    m = dict(sc["m"], kf_valid=sc["m"]["kf_valid"].copy())
    m["kf_valid"][list(invalid)] = 0
    NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
    md, bd, rk, sizes = upload(torch, with_point_arrays(m), sc["ba"], sc["mp_ref_kf"], NMP, NOBS + 30000)
    kf_desc = torch.from_numpy(sc["kf_desc"]).cuda()
    refresh(ctx, md, bd, rk, kf_desc, sizes)
    NKF = sizes[1]
    cov = covis.covis_alloc(NKF, NKF)
    view, _ = map_grow.map_views(md, bd, sizes)
    for k in range(NKF):
        covis.covis_update(ctx, covis._view(view), cov, k)
    rng = np.random.default_rng(5)
    stats = map_stats.map_stats_alloc(NMP, 4)
    stats["visible"] = torch.from_numpy(rng.integers(1, 50, NMP).astype(np.int32)).cuda()
    stats["found"] = torch.from_numpy(rng.integers(1, 50, NMP).astype(np.int32)).cuda()
    return dict(md=md, bd=bd, rk=rk, sizes=sizes, kf_desc=kf_desc, cov=cov, stats=stats, rep=torch.full((NMP,), -1, dtype=torch.int32, device="cuda"))


def _host(torch, s, sizes):
    torch.cuda.synchronize()
    mm, bb = map_grow.map_views(s["md"], s["bd"], sizes)
    out = {k: mm[k].cpu().numpy() for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf", "mp_pos") + POINT_KEYS}
    out.update(obs_feat=bb["obs_feat"].cpu().numpy(), mp_ref_kf=s["rk"].cpu().numpy(), visible=s["stats"]["visible"].cpu().numpy(),
               found=s["stats"]["found"].cpu().numpy(), mp_replaced=s["rep"].cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in s["cov"].items()})
    return out


def _split_route(torch, ctx, cam, s, kf_row, kf_idx):
    """searchInNeighbors the way a host does it today: the graph and the two lists in numpy from read-backs (tests/covis_ref.py), one
    fuse_observations_from_map per target by hand, the refreshes through masks made on the host"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = {k: v.cpu().numpy() for k, v in s["cov"].items()}
    sizes = s["sizes"]
    NMP, NKF = sizes[0], sizes[1]
    kf_valid = s["md"]["kf_valid"].cpu().numpy()
    targets = R.Model.from_rows(g).fuse_targets(kf_row, kf_valid)
    snapshot = s["md"]["kf_mp"][kf_row].cpu().numpy().copy()
    counts = []

    def refresh_rows(rows, what):
        valid = s["md"]["mp_valid"].cpu().numpy()[:NMP]
        mask = np.zeros(NMP, np.uint8)
        rows = np.asarray(rows, np.int64)
        mask[rows[(rows >= 0) & (rows < NMP)]] = 1
        mm, bb = map_grow.map_views(s["md"], s["bd"], sizes)
        api.update_map_points(ctx, dict(twc=bb["kf_twc"], valid=mm["kf_valid"], oct=bb["kf_oct"], desc=s["kf_desc"]),
                              dict(pos=mm["mp_pos"], valid=T(mask & (valid != 0)), ref_kf=s["rk"], obs_ptr=mm["obs_ptr"], obs_kf=mm["obs_kf"], obs_feat=bb["obs_feat"]),
                              dict(desc=mm["mp_desc"], normal=mm["mp_normal"], max_dist=mm["mp_max_dist"], min_dist=mm["mp_min_dist"]), what=what)

    def fuse(kf, cand):
        nonlocal sizes
        r = map_grow.fuse_observations_from_map(ctx, cam, s["md"], s["bd"], dict(desc=s["kf_desc"]), kf, T(np.asarray(cand, np.int32)), sizes=sizes)
        assert r["status"] == 0
        sizes = r["sizes"]
        counts.append((r["n_fused"], r["n_attached"], r["n_replaced"]))
        if r["n_replaced"]:
            refresh_rows(r["repl_tgt"].cpu().numpy(), 1)
            map_stats.map_stats_merge(ctx, s["stats"], NMP, r["repl_src"], r["repl_tgt"])
            frame_step.note_replaced(ctx, s["rep"], r["repl_src"], r["repl_tgt"])

    for k in targets:
        fuse(k, snapshot)
    now = {k: s["md"][k].cpu().numpy() for k in ("kf_mp", "mp_valid")}
    cand = R.fuse_candidates(dict(now, kf_mp=now["kf_mp"][:NKF], mp_valid=now["mp_valid"][:NMP]), targets, kf_idx)
    fuse(kf_row, cand)
    refresh_rows(s["md"]["kf_mp"][kf_row].cpu().numpy(), 3)
    h = {k: s["md"][k].cpu().numpy() for k in ("kf_mp", "mp_valid", "obs_ptr", "obs_kf", "kf_valid")}
    m_now = dict(kf_mp=h["kf_mp"][:NKF], mp_valid=h["mp_valid"][:NMP], obs_ptr=h["obs_ptr"][:NMP + 1], obs_kf=h["obs_kf"][:sizes[2]], kf_valid=h["kf_valid"])
    conn = R.rows_update(g, m_now, kf_row, 256)
    s["cov"] = {k: T(v) for k, v in g.items()}
    s["sizes"] = sizes
    return targets, cand, counts, conn


@pytest.mark.parametrize("invalidate", [False, True], ids=["as_it_is", "two_neighbours_invalid"])
def test_composite_equals_the_split_route(gpu, map_v1, gt_sync, invalidate):
    torch, ctx = gpu
    cam = api.Camera()
    sc = GS.geo_scene(*map_v1, gt_sync["V1_01_easy"])
    K, kf_idx = sc["kf_row"], 5
    invalid = ()
    if invalidate:  # the second and the fourth of the key-frame's neighbours, as the graph of the intact scene lists them
        s0 = _scene(torch, ctx, sc)
        first = s0["cov"]["cov_kf"][K].cpu().numpy()
        assert int(s0["cov"]["cov_nord"][K]) >= 4
        invalid = (int(first[1]), int(first[3]))
    a, b = _scene(torch, ctx, sc, invalid), _scene(torch, ctx, sc, invalid)
    r = covis.search_in_neighbors_from_map(ctx, cam, a["md"], a["bd"], a["cov"], dict(desc=a["kf_desc"]), K, kf_idx, stats=a["stats"],
                                           mp_replaced=a["rep"], mp_ref_kf=a["rk"], sizes=a["sizes"])
    targets, cand, counts, conn = _split_route(torch, ctx, cam, b, K, kf_idx)
    print("targets", targets, "candidates", len(cand), "(fused, attached, replaced) per fuse", counts)
    assert r["status"] == 0 and r["tgt_kf"] == targets and r["n_cand"] == len(cand) and r["sizes"] == b["sizes"]
    assert list(zip(r["n_fused"], r["n_attached"], r["n_replaced"])) == counts
    assert len(targets) >= 3 and len(cand) > 50 and not set(targets) & set(invalid)
    assert sum(c[1] for c in counts) >= 1 and sum(c[2] for c in counts) >= 1  # the fuses attached and replaced
    ha, hb = _host(torch, a, r["sizes"]), _host(torch, b, b["sizes"])
    alive = hb["mp_valid"] != 0  # (update_map_points leaves the rows of an invalid point as they are)
    for k in ha:
        x, y = (ha[k][alive], hb[k][alive]) if k in POINT_KEYS else (ha[k], hb[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    same_out({k: v.cpu().numpy() for k, v in r["conn"].items()}, conn, "the closing update")
    assert not (ha["mp_replaced"] == -1).all()
