"""The key-frame kernels on the hand-built cases of tests/keyframe_cases.py: every case through every path of its kernel must give the
output the case DECLARES (tests/test_keyframe_cases.py holds the C++ oracle and oracle/numpy_ref.py to the same outputs on the CPU) and
the oracle's numbers: integers and ids exact, points to atol 1e-9, chi2 to rtol 1e-8 / atol 1e-10.
  gl_search2d: view_threads 256 and 1024, view_slot_lds default and 4 (the list spills after four slots), nfeat given and NULL; every
    view alone, and with the other views of its map (or, where its map has one view, a view that looks away) in one call, forward and
    reversed.
  the point kernels: every case alone (N = 1); all cases of one map in one call, forward and reversed (the row, the place in the wave and
    the neighbours in it change); and as the last row of a call of six (the last wave holds two rows of its four).
  gl_check_map_association with B = 3: the case in frames 0 and 2, a skipped feature between (B N = 3 is no multiple of 4).
  the chain: search2d feeds gl_check_map_association and gl_create_map_points on the device.
The regime scenes are compared with the oracle bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import keyframe_cases as kc
from tests.gpu_helpers import T

pytestmark = pytest.mark.gpu

NAMES = sorted(kc.CASES)
VIEW = [n for n in NAMES if kc.CASES[n].call == "view"]
POINT = [n for n in NAMES if kc.CASES[n].call != "view"]
AWAY = np.array([0, 1, 0, 0, 0, 0, 0], np.float64)  # half a turn about y: looks away from everything in front of the identity
KEYS = {"pt": kc.PT_KEYS, "cma": kc.CMA_KEYS, "tri": kc.TRI_KEYS, "cmp": kc.CMP_KEYS}
CHI2 = ("c2p", "c2s")
_ref, _gmm = {}, {}


def reference(oracle, key, call, data):
    """the oracle's outputs of a case: computed once, shared, never written to"""
    if key not in _ref:
        _ref[key] = kc.run(oracle, call, data)
        for v in _ref[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _ref[key]


def map_key(d):
    return (d["mean"].tobytes(), d["cov"].tobytes())


def gmm_of(ctx, d):
    k = map_key(d)
    if k not in _gmm:
        _gmm[k] = api.GMM(ctx, d["mean"], d["cov"].reshape(-1, 9))
    return _gmm[k]


# ---- gl_search2d ------------------------------------------------------------------------------------------------------------------------
def dev_views(torch, ctx, datas, give_nfeat):
    """views of one map (one camera, k, N and view_cap) in one call -> per view the outputs of keyframe_cases.run"""
    d0 = datas[0]
    N, k = d0["uv"].shape[0], d0["k"]
    cap = d0["cap"]
    nfeat = None
    if give_nfeat or any(d.get("nfeat") is not None for d in datas):
        nfeat = T(torch, np.array([N if d.get("nfeat") is None else d["nfeat"] for d in datas], np.int32))
    cand, ncand, vids, nview = gmm_of(ctx, d0).search2d(api.Camera(**d0["cam"]), T(torch, np.stack([d["pose"] for d in datas])),
                                                        T(torch, np.stack([d["uv"] for d in datas]).reshape(len(datas), N, 2)), nfeat, k=k, view_cap=cap)
    torch.cuda.synchronize()
    cand, ncand, vids, nview = cand.cpu().numpy(), ncand.cpu().numpy(), vids.cpu().numpy(), nview.cpu().numpy()
    return [dict(ids=vids[b], nview=int(nview[b]), cand=cand[b], ncand=ncand[b]) for b in range(len(datas))]


def with_cap(oracle, name, data):
    r = reference(oracle, name, "view", data)
    return dict(data, cap=len(r["ids"])), r


def check_view(name, o, r, want=None):
    for k in ("ids", "nview", "cand", "ncand"):
        assert np.array_equal(np.asarray(o[k]), np.asarray(r[k])), (name, k, o[k], r[k])
        if want is not None and k in want:
            assert np.array_equal(np.asarray(o[k]), np.asarray(want[k])), (name, k, "declared", o[k], want[k])


@pytest.mark.parametrize("slot_lds", [None, 4])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", VIEW)
def test_view_case_alone(gpu, oracle, opt, name, threads, slot_lds):
    torch, ctx = gpu
    opt("view_threads", threads)
    if slot_lds:
        opt("view_slot_lds", slot_lds)
    c = kc.CASES[name]
    d, r = with_cap(oracle, name, c.data)
    for give in ((True,) if d.get("nfeat") is not None else (False, True)):
        check_view(name, dev_views(torch, ctx, [d], give)[0], r, c.want)


def _view_groups():
    g = {}
    for n in VIEW:
        d = kc.CASES[n].data
        g.setdefault(map_key(d) + (tuple(sorted(d["cam"].items())), d["k"], d["uv"].shape[0], d["view_cap"]), []).append(n)
    return list(g.values())


VIEW_GROUPS = _view_groups()


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("group", VIEW_GROUPS, ids=[g[0] for g in VIEW_GROUPS])
def test_views_of_one_map_in_one_call(gpu, oracle, opt, group, threads, order):
    torch, ctx = gpu
    opt("view_threads", threads)
    items = [(n,) + with_cap(oracle, n, kc.CASES[n].data) for n in group]
    if len(items) == 1:  # a view that sees nothing, before and after
        n, d, r = items[0]
        away = dict(d, pose=AWAY)
        ra = reference(oracle, n + "|away", "view", dict(away, view_cap=d["cap"]))
        items = [(n + "|away", away, ra), items[0], (n + "|away", away, ra)]
    cap = max(d["cap"] for _, d, _ in items)
    items = [(n, dict(d, cap=cap), r) for n, d, r in items]
    if order == "reversed":
        items = items[::-1]
    outs = dev_views(torch, ctx, [d for _, d, _ in items], False)
    for (n, d, r), o in zip(items, outs):
        L = len(r["ids"])
        assert (o["ids"][L:] == -1).all(), n
        check_view(n, dict(o, ids=o["ids"][:L]), r, kc.CASES[n].want if n in kc.CASES else None)


@pytest.mark.parametrize("slot_lds", [None, 24])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", sorted(kc.REGIMES))
def test_regime_scene(gpu, oracle, opt, name, threads, slot_lds):
    torch, ctx = gpu
    opt("view_threads", threads)
    if slot_lds:
        opt("view_slot_lds", slot_lds)
    d, r = with_cap(oracle, "regime|" + name, kc.REGIMES[name]["data"])
    check_view(name, dev_views(torch, ctx, [d, dict(d, pose=AWAY), d], False)[0], r)
    check_view(name, dev_views(torch, ctx, [d, dict(d, pose=AWAY), d], True)[2], r)


# ---- the point kernels ------------------------------------------------------------------------------------------------------------------
def dev_point(torch, ctx, call, d, rows):
    """one call on the rows (dicts of the per-row arrays of KEYS[call], each of one row) of the map, camera and parameters of d"""
    g, cam, prm = gmm_of(ctx, d), api.Camera(**d["cam"]), api.Params(**d.get("prm", {}))
    cat = lambda k: T(torch, np.concatenate([r[k] for r in rows]))
    if call == "pt":
        res, c2p, c2s, est = api.optimize_point(ctx, g, cam, prm, *[cat(k) for k in kc.PT_KEYS])
        torch.cuda.synchronize()
        return dict(res=res.cpu().numpy(), c2p=c2p.cpu().numpy(), c2s=c2s.cpu().numpy(), est=est.cpu().numpy())
    if call == "cma":  # one frame of len(rows) features
        pts = cat("pts")[None].contiguous()
        out = api.check_map_association(ctx, g, cam, prm, T(torch, d["pose"][None]), pts, cat("uvr")[None].contiguous(), cat("oct")[None].contiguous(),
                                        cat("cand")[None].contiguous(), cat("ncand")[None].contiguous())
        torch.cuda.synchronize()
        return dict(out=out.cpu().numpy()[0], pts=pts.cpu().numpy()[0])
    if call == "tri":
        x = cat("x3d")
        out = api.optimize_triangulation(ctx, g, cam, prm, x, *[cat(k) for k in kc.TRI_KEYS[1:]])
        torch.cuda.synchronize()
        return dict(out=out.cpu().numpy(), x=x.cpu().numpy())
    x, t, c = api.create_map_points(ctx, g, cam, prm, *[cat(k) for k in kc.CMP_KEYS], scale_factor=d.get("scale_factor", 1.2))
    torch.cuda.synchronize()
    return dict(x=x.cpu().numpy(), type=t.cpu().numpy(), comp=c.cpu().numpy())


def row_of(call, d):
    return {k: d[k] for k in KEYS[call] if not (call == "cma" and k == "pose")}


def check_point(name, call, o, i, r, want, data):
    """row i of the device's outputs o against the oracle's outputs r of the case (one row) and the declared output"""
    for k, v in r.items():
        if v.dtype.kind in "iu":
            assert o[k][i] == v[0], (name, k, o[k][i], v[0])
        elif k in CHI2:
            np.testing.assert_allclose(o[k][i], v[0], rtol=1e-8, atol=1e-10, err_msg="%s %s" % (name, k))
        else:
            np.testing.assert_allclose(o[k][i], v[0], rtol=0, atol=1e-9, err_msg="%s %s" % (name, k))
    pin = {"pt": "pts", "cma": "pts", "tri": "x3d"}.get(call)
    pout = {"pt": "est", "cma": "pts", "tri": "x"}.get(call)
    for k, w in want.items():
        if k == "moved":
            assert bool((o[pout][i] != data[pin][0]).any()) == bool(w[0]), (name, "moved")
            if not w[0]:
                assert np.array_equal(o[pout][i], data[pin][0]), (name, "untouched")
        elif k == "z_side":
            assert np.sign(o[pout][i][2] - data[pin][0][2]) == w, (name, "z_side")
        elif k == "xzero":
            assert bool((o["x"][i] == 0).all()) == bool(w[0]), (name, "xzero")
        elif k in CHI2:
            assert o[k][i] == w[0], (name, k, o[k][i])
        else:
            assert o[k][i] == w[0], (name, k, "declared", o[k][i], w[0])


@pytest.mark.parametrize("name", POINT)
def test_point_case_alone(gpu, oracle, name):
    torch, ctx = gpu
    c = kc.CASES[name]
    o = dev_point(torch, ctx, c.call, c.data, [row_of(c.call, c.data)])
    check_point(name, c.call, o, 0, reference(oracle, name, c.call, c.data), c.want, c.data)


@pytest.mark.parametrize("name", POINT)
def test_point_case_in_the_last_partial_wave(gpu, oracle, name):
    """six rows, the case the last: the second wave of the 16-lane kernels holds two rows of its four"""
    torch, ctx = gpu
    c = kc.CASES[name]
    row = row_of(c.call, c.data)
    o = dev_point(torch, ctx, c.call, c.data, [row] * 6)
    r = reference(oracle, name, c.call, c.data)
    for i in (0, 5):
        check_point(name, c.call, o, i, r, c.want, c.data)


def _point_groups():
    g = {}
    for n in POINT:
        c = kc.CASES[n]
        d = c.data
        shape = tuple(d[k].shape[1:] for k in KEYS[c.call] if d[k].ndim > 1)
        g.setdefault((c.call,) + map_key(d) + (tuple(sorted(d["cam"].items())), tuple(sorted(d.get("prm", {}).items())), d.get("scale_factor"), shape), []).append(n)
    return [v for v in g.values() if len(v) > 1]


POINT_GROUPS = _point_groups()


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("group", POINT_GROUPS, ids=[g[0] for g in POINT_GROUPS])
def test_point_cases_of_one_map_in_one_call(gpu, oracle, group, order):
    torch, ctx = gpu
    names = group if order == "forward" else group[::-1]
    c0 = kc.CASES[names[0]]
    o = dev_point(torch, ctx, c0.call, c0.data, [row_of(c0.call, kc.CASES[n].data) for n in names])
    for i, n in enumerate(names):
        c = kc.CASES[n]
        check_point(n, c.call, o, i, reference(oracle, n, c.call, c.data), c.want, c.data)


def test_point_groups_cover_the_kernels():
    calls = {kc.CASES[g[0]].call for g in POINT_GROUPS}
    assert calls == {"pt", "cma", "tri", "cmp"} and max(len(g) for g in POINT_GROUPS) >= 16  # more than one wave of rows


CMA = [n for n in POINT if kc.CASES[n].call == "cma"]


@pytest.mark.parametrize("name", CMA)
def test_check_map_association_three_frames(gpu, oracle, name):
    """the case in frames 0 and 2 of B = 3 (another pose between, its feature skipped): B N = 3 rows, one partial wave"""
    torch, ctx = gpu
    c = kc.CASES[name]
    d = c.data
    g, cam, prm = gmm_of(ctx, d), api.Camera(**d["cam"]), api.Params(**d.get("prm", {}))
    rep = lambda a: np.stack([a, a, a])
    octv = rep(d["oct"])
    octv[1] = -1
    pts = T(torch, rep(d["pts"]))
    out = api.check_map_association(ctx, g, cam, prm, T(torch, np.stack([d["pose"], AWAY, d["pose"]])), pts, T(torch, rep(d["uvr"])), T(torch, octv),
                                    T(torch, rep(d["cand"])), T(torch, rep(d["ncand"])))
    torch.cuda.synchronize()
    out, pts = out.cpu().numpy(), pts.cpu().numpy()
    r = reference(oracle, name, "cma", d)
    for b in (0, 2):
        check_point(name, "cma", dict(out=out[b], pts=pts[b]), 0, r, c.want, d)
    assert out[1, 0] == -1 and np.array_equal(pts[1], d["pts"])


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.CHAINS))
def test_chain(gpu, oracle, name):
    """search2d's tables stay on the device and feed the point kernel"""
    torch, ctx = gpu
    ch = kc.CHAINS[name]
    d, vs = ch["data"], ch["views"]
    g, cam, prm = gmm_of(ctx, d), api.Camera(**d["cam"]), api.Params(**d.get("prm", {}))
    cand, ncand, _, _ = g.search2d(cam, T(torch, np.stack([v["pose"] for v in vs])), T(torch, np.stack([v["uv"] for v in vs])), None, k=vs[0]["k"])
    r = reference(oracle, "chain|" + name, ch["call"], d)
    if ch["call"] == "cma":
        pts = T(torch, d["pts"][None])
        out = api.check_map_association(ctx, g, cam, prm, T(torch, d["pose"][None]), pts, T(torch, d["uvr"][None]), T(torch, d["oct"][None]), cand, ncand)
        torch.cuda.synchronize()
        o = dict(out=out.cpu().numpy()[0], pts=pts.cpu().numpy()[0])
    else:
        a = [T(torch, d[k]) for k in kc.CMP_KEYS[:8]]
        x, t, c = api.create_map_points(ctx, g, cam, prm, *a, cand[0].contiguous(), ncand[0].contiguous(), cand[1].contiguous(), ncand[1].contiguous(),
                                        scale_factor=d["scale_factor"])
        torch.cuda.synchronize()
        o = dict(x=x.cpu().numpy(), type=t.cpu().numpy(), comp=c.cpu().numpy())
    for b, want in enumerate(ch["cand"]):
        assert np.array_equal(cand.cpu().numpy()[b], want), (name, "cand", b)
    check_point(name, ch["call"], o, 0, r, ch["want"], d)
