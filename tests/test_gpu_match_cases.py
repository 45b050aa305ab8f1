"""The matcher kernels on the hand-built cases of tests/match_cases.py: every case through every path of its kernel must give the
output the case DECLARES (tests/test_match_cases.py holds the C++ oracle and oracle/numpy_ref.py to the same outputs on the CPU) -
matches, counts and, for the fuse search, best distances, exact.
  searchByProjection (local map): match_desc_lds 0 / 1, the record walk and the general walk (match_cases.with_double_feature: one far
    feature with non-float coordinates switches the whole frame over, so every case runs both), gl_search_by_projection and - the
    cases that can be said as 3-D points (match_cases.as_points3d says which cannot, and why) - gl_search_local_points;
  searchByProjection (last frame): match_desc_lds 0 / 1, both walks;  the fuse search: fuse_records 0 / 1, both walks;
  searchForTriangulation, searchByBoW: their one path.
Every case runs alone (B = 1) and as the middle frame of a batch of three whose neighbours are synth frames of another size (which must
still equal the oracle).  The 512 x 384 cases run with that image size in the camera.  The regime scenes are compared with the oracle
bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api, synth
from tests import match_cases as MC
from tests.test_gpu_match import FKEYS, FUSE_KEYS, KEYS, _pack_bow, _pack_fuse, _pack_pairs

pytestmark = pytest.mark.gpu

PK = ("pose_cw", "t_wc", "pos", "normal", "max_dist", "min_dist", "cand")
PAD = {"feat_ur": -1.0, "feat_oct": -1}  # a padding slot: no feature (octave -1), no map point (valid 0)
DTYPE = {"feat_uv": np.float64, "feat_ur": np.float32, "feat_oct": np.int32, "feat_angle": np.float32, "feat_desc": np.uint8, "feat_taken": np.uint8,
         "mp_uvr": np.float64, "mp_level": np.int32, "mp_viewcos": np.float64, "mp_valid": np.uint8, "mp_desc": np.uint8, "pose_cw": np.float64,
         "pose_lw": np.float64, "last_pt": np.float64, "last_valid": np.uint8, "last_oct": np.int32, "last_angle": np.float32, "last_desc": np.uint8,
         "t_wc": np.float64, "pos": np.float64, "normal": np.float64, "max_dist": np.float32, "min_dist": np.float32, "cand": np.uint8}


def cam_of(size):
    cam = api.Camera()
    cam.width, cam.height = size
    return cam


def pack(torch, datas, keys):
    """frames of different sizes as one batch: every array padded to the largest (pose-like arrays have one shape)"""
    out = []
    for k in keys:
        arrs = [np.asarray(d[k], DTYPE[k]) for d in datas]
        shape = tuple(max(a.shape[i] for a in arrs) for i in range(arrs[0].ndim))
        t = np.full((len(arrs),) + shape, PAD.get(k, 0), DTYPE[k])
        for b, a in enumerate(arrs):
            t[(b,) + tuple(slice(0, s) for s in a.shape)] = a
        out.append(torch.from_numpy(t).cuda())
    return out


def gpu_run(torch, ctx, matcher, datas, kw, size=(MC.W0, MC.H0)):
    """-> per frame (match, count, best_dist or None), cut to the frame's own size"""
    if matcher == "proj":
        m, n = api.search_by_projection(ctx, cam_of(size), *pack(torch, datas, KEYS), **kw)
        lens = [len(d["feat_oct"]) for d in datas]
    elif matcher == "local":
        a = pack(torch, datas, KEYS[:5] + PK + ("mp_desc",))
        m, n, _ = api.search_local_points(ctx, cam_of(size), *a, **kw)
        lens = [len(d["feat_oct"]) for d in datas]
    elif matcher == "frame":
        m, n = api.search_by_projection_frame(ctx, cam_of(size), *pack(torch, datas, FKEYS), **kw)
        lens = [len(d["feat_oct"]) for d in datas]
    elif matcher == "tri":
        k1, k2, fm, ep = _pack_pairs(torch, datas)
        m, n = api.search_for_triangulation(ctx, k1, k2, fm, ep, **kw)
        lens = [len(d["kf1"]["oct"]) for d in datas]
    elif matcher == "bow":
        kf, fr = _pack_bow(torch, datas)
        m, n = api.search_by_bow(ctx, kf, fr, **kw)
        lens = [len(d[1]["angle"]) for d in datas]
    else:
        bi, bd = api.fuse_search(ctx, cam_of(size), *_pack_fuse(torch, datas), **kw)
        torch.cuda.synchronize()
        bi, bd = bi.cpu().numpy(), bd.cpu().numpy()
        return [(bi[b, :len(d["mp_valid"])], int((bi[b, :len(d["mp_valid"])] >= 0).sum()), bd[b, :len(d["mp_valid"])]) for b, d in enumerate(datas)]
    torch.cuda.synchronize()
    m, n = m.cpu().numpy(), n.cpu().numpy()
    assert all((m[b, l:] == -1).all() for b, l in enumerate(lens)), "a padding slot has a match"
    return [(m[b, :l], int(n[b]), None) for b, l in enumerate(lens)]


def equal(got, want_m, want_n, want_d=None):
    return np.array_equal(got[0], want_m) and got[1] == want_n and (want_d is None or np.array_equal(got[2], want_d))


class Neighbours:
    """two synth frames of another size per (matcher, image size) and the oracle's answer on them per argument set, computed once"""

    def __init__(self, oracle):
        self.o, self.frames, self.ref = oracle, {}, {}

    def get(self, matcher, size, kw):
        key = (matcher, size)
        if key not in self.frames:
            cam = cam_of(size)
            if matcher == "proj":
                f = [synth.synth_match_frame(300, 200, 51, *size, dup_frac=0.5), synth.synth_match_frame(150, 260, 52, *size, float_uv=False)]
            elif matcher == "local":
                f = [synth.synth_local_points_frame(300, 500, 53, cam), synth.synth_local_points_frame(120, 700, 54, cam, float_uv=False)]
            elif matcher == "frame":
                f = [synth.synth_motion_frames(300, 250, 55, cam), synth.synth_motion_frames(200, 300, 56, cam, "forward", float_uv=False)]
            elif matcher == "tri":
                f = [synth.synth_tri_search_pair(300, 350, 57, cam, n_nodes=40), synth.synth_tri_search_pair(90, 70, 58, cam, n_nodes=6, pad=1)]
            elif matcher == "bow":
                f = [synth.synth_bow_pair(300, 350, 59, cam, n_nodes=40), synth.synth_bow_pair(90, 70, 60, cam, n_nodes=6)]
            else:
                f = [synth.synth_fuse_frame(300, 260, 61, *size), synth.synth_fuse_frame(120, 400, 62, *size, float_coords=True)]
            self.frames[key] = f
        kk = key + tuple(sorted(kw.items()))
        if kk not in self.ref:
            self.ref[kk] = [self.one(matcher, size, d, kw) for d in self.frames[key]]
        return self.frames[key], self.ref[kk]

    def one(self, matcher, size, d, kw):
        if matcher == "local":
            uvr, lvl, vc, dd, iv, n = self.o.project_map_points(cam_of(size), **{k: d[k] for k in PK})
            m, n = self.o.search_by_projection(size[0], size[1], d["feat_uv"], d["feat_ur"], d["feat_oct"], d["feat_desc"], d["feat_taken"], uvr, lvl, vc, iv,
                                               d["mp_desc"], **kw)
            return m, n, None
        return MC.run(self.o, matcher, d, kw)


@pytest.fixture(scope="module")
def neighbours(oracle):
    return Neighbours(oracle)


def run_cases(torch, ctx, nb, matcher, cases, variant=None, kernel=None):
    """every case alone and in the middle of a batch -> the list of what differed from the declared output"""
    kernel = kernel or matcher
    bad, ran = [], 0
    for c in cases:
        data, want = variant(c) if variant else (c.data, c.want)
        alone = gpu_run(torch, ctx, kernel, [data], c.kw, c.size)[0]
        if not equal(alone, want, c.n, c.dist):
            bad.append("%s alone: %s %s, declared %s %s" % (c.name, alone[0].tolist(), None if alone[2] is None else alone[2].tolist(), want.tolist(),
                                                               None if c.dist is None else c.dist.tolist()))
        (f0, f1), (r0, r1) = nb.get(kernel, c.size, c.kw)
        got = gpu_run(torch, ctx, kernel, [f0, data, f1], c.kw, c.size)
        if not equal(got[1], want, c.n, c.dist):
            bad.append("%s in a batch: %s, declared %s" % (c.name, got[1][0].tolist(), want.tolist()))
        if not (equal(got[0], *r0) and equal(got[2], *r1)):
            bad.append("%s: a neighbour frame of its batch differs from the oracle" % c.name)
        ran += 1
    return bad, ran


def of(matcher):
    return [c for c in MC.CASES.values() if c.matcher == matcher]


WALKS = {"records": None, "doubles": MC.with_double_feature}


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("lds", [0, 1])
def test_search_by_projection_cases(gpu, opt, neighbours, lds, walk):
    torch, ctx = gpu
    opt("match_desc_lds", lds)
    bad, ran = run_cases(torch, ctx, neighbours, "proj", of("proj"), WALKS[walk])
    assert not bad, "\n".join(bad)
    assert ran >= 60


@pytest.mark.parametrize("lds", [0, 1])
def test_search_local_points_cases(gpu, opt, neighbours, lds):
    """the local-map cases as 3-D points through gl_project_map_points -> the search, in one call"""
    torch, ctx = gpu
    opt("match_desc_lds", lds)

    def variant(c):
        d = dict(c.data)
        d.update(MC.as_points3d(c))
        return d, c.want
    cases = [c for c in of("proj") if MC.as_points3d(c) is not None]
    bad, ran = run_cases(torch, ctx, neighbours, "proj", cases, variant, kernel="local")
    assert not bad, "\n".join(bad)
    assert ran >= 40


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("lds", [0, 1])
def test_search_by_projection_frame_cases(gpu, opt, neighbours, lds, walk):
    torch, ctx = gpu
    opt("match_desc_lds", lds)
    bad, ran = run_cases(torch, ctx, neighbours, "frame", of("frame"), WALKS[walk])
    assert not bad, "\n".join(bad)
    assert ran >= 50


def test_search_for_triangulation_cases(gpu, neighbours):
    torch, ctx = gpu
    bad, ran = run_cases(torch, ctx, neighbours, "tri", of("tri"))
    assert not bad, "\n".join(bad)
    assert ran >= 35


def test_search_by_bow_cases(gpu, neighbours):
    torch, ctx = gpu
    bad, ran = run_cases(torch, ctx, neighbours, "bow", of("bow"))
    assert not bad, "\n".join(bad)
    assert ran >= 40


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("records", [0, 1])
def test_fuse_search_cases(gpu, opt, neighbours, records, walk):
    torch, ctx = gpu
    opt("fuse_records", records)
    bad, ran = run_cases(torch, ctx, neighbours, "fuse", of("fuse"), WALKS[walk])
    assert not bad, "\n".join(bad)
    assert ran >= 20


# ---- the regime scenes: the oracle's bits ----------------------------------------------------------------------------------------------
def check_regime(torch, ctx, oracle, matcher, data, kw):
    ref = MC.run(oracle, matcher, data, kw)
    got = gpu_run(torch, ctx, matcher, [data], kw)[0]
    assert equal(got, *ref), (matcher, int((got[0] != ref[0]).sum()), got[1], ref[1])
    return ref


@pytest.mark.parametrize("n_feat,strict", MC.WIDE_WINDOWS)
@pytest.mark.parametrize("lds", [0, 1])
def test_wide_window(gpu, oracle, opt, lds, n_feat, strict):
    """256 / 257 / 300 candidates in one window, six queries that compete for the last ones in visiting order, both walks.  256 is the
    most a record keys (the queries 1 and 2 then decide from their records, whose best key sits at position 255); with 257 the candidate
    at position 256 does not fit the 8 bits of a record and the queries walk in every round"""
    torch, ctx = gpu
    opt("match_desc_lds", lds)
    for fn, matcher in ((MC.wide_window, "proj"), (MC.wide_window_frame, "frame")):
        data, kw, order = fn(n_feat, strict=strict)
        ref = check_regime(torch, ctx, oracle, matcher, data, kw)
        assert ref[1] == 6
        if strict:  # query 0 ends on the LAST candidate in visiting order: position 255 (keyed) / 256 (not keyed)
            assert ref[0][order[n_feat - 1]] == 0 and ref[0][order[n_feat - 3]] == 2
        c = MC.Case("wide_window", matcher, "proj.tie", "", data, ref[0], kw)
        d2, want = MC.with_double_feature(c)
        assert equal(gpu_run(torch, ctx, matcher, [d2], kw)[0], want, 6)


@pytest.mark.parametrize("fuv", [True, False])
@pytest.mark.parametrize("lds", [0, 1])
def test_relist_overflow(gpu, oracle, opt, lds, fuv):
    """the conflict chain with 2 500 map points: from the third round on more queries walk again than the list holds (2 048 in the
    1 024-thread shape), the rest walk in place"""
    torch, ctx = gpu
    opt("match_desc_lds", lds)
    data, kw = MC.conflict_chain(float_uv=fuv)
    ref = check_regime(torch, ctx, oracle, "proj", data, kw)
    assert ref[1] == 40 and ref[0].tolist() == list(range(40))


@pytest.mark.parametrize("matcher,args", [("bow", {}), ("bow", {"rejecting": 5}), ("tri", {}), ("tri", {"tie": True})])
def test_deep_chain(gpu, oracle, matcher, args):
    """12 queries of one node that all prefer the same 12 partners in the same order: from the fourth on a query has lost its three
    cached keys and walks again"""
    torch, ctx = gpu
    data, kw = MC.deep_chain(matcher, **args)
    ref = check_regime(torch, ctx, oracle, matcher, data, kw)
    assert ref[1] == (8 if args.get("rejecting") else 12)


@pytest.mark.parametrize("n2,winner,best,second,ratio", MC.BIG_NODES)
@pytest.mark.parametrize("matcher", ["bow", "tri"])
def test_big_node(gpu, oracle, matcher, n2, winner, best, second, ratio):
    """a node of more than 1 024 partners: the partners past position 1 023 cannot be keyed (the sequential walk); 1 024 is the last
    keyed size"""
    torch, ctx = gpu
    data, kw = MC.big_node(matcher, n2=n2, winner=winner, best=best, second=second, nn_ratio=ratio)
    ref = check_regime(torch, ctx, oracle, matcher, data, kw)
    assert (winner > 1023) == (n2 > 1024)
    if matcher == "bow":  # the first query gets the partner at position `winner` of the node's list
        assert ref[0][winner] == 0 and ref[0][winner - 2] == 1
    else:
        assert ref[0][:2].tolist() == [winner, winner - 2]


# ---- the stated capacities -----------------------------------------------------------------------------------------------------------
# Each entry point at the largest sizes its GL_REQUIRE states (match_cases.capacity_scenes: projection 3 072 / 4 096, triangulation and BoW
# 4 096 / 4 096, fuse 16 384), on synth scenes with dense conflicts, in every launch shape.  What happens at capacity: every call succeeds
# (no error status) and gives the oracle's bits - asserted below.  tests/test_match_cases.py pins the oracle's counts on the same scenes.
SHAPES = {"proj": ("match_desc_lds", (0, 1)), "frame": ("match_desc_lds", (0, 1)), "fuse": ("fuse_records", (0, 1)), "tri": (None, (0,)), "bow": (None, (0,))}


@pytest.fixture(scope="module")
def capacity(oracle):
    """scene -> (matcher, data, kw, the oracle's result), computed once"""
    return {k: (m, d, kw, MC.run(oracle, m, d, kw)) for k, (m, d, kw) in MC.capacity_scenes().items()}


@pytest.mark.parametrize("matcher", list(SHAPES))
def test_capacity_gives_the_oracles_bits(gpu, opt, capacity, matcher):
    torch, ctx = gpu
    option, values = SHAPES[matcher]
    ran = 0
    for name, (m, data, kw, ref) in capacity.items():
        if m != matcher:
            continue
        for v in values:
            if option:
                opt(option, v)
            got = gpu_run(torch, ctx, matcher, [data], kw)[0]  # (an error status raises api.GLError: the call must succeed)
            assert equal(got, *ref), (name, option, v, int((got[0] != ref[0]).sum()), got[1], ref[1])
            ran += 1
    assert ran >= 2


def test_one_above_capacity_is_an_error_that_writes_nothing(gpu):
    """NF / NP / N1 / N2 one above what an entry point states: an error status, gl_last_error_string() names the capacity, and the output
    buffers still hold the marker they were filled with"""
    torch, ctx = gpu
    import ctypes as C
    from gmmloc_amd import _lib
    lib, cam, P = ctx.lib, api.Camera().c(), api._ptr
    Z = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")
    f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8

    def feats(NF):
        return [Z(f64, 1, NF, 2), Z(f32, 1, NF), Z(i32, 1, NF), Z(u8, 1, NF, 32)]

    def kf(N, with_geometry):
        a = [Z(f64, 1, N, 2), Z(f32, 1, N), Z(i32, 1, N)] if with_geometry else []
        return a + [Z(f32, 1, N), Z(u8, 1, N, 32), Z(u8, 1, N), Z(i32, 1), Z(i32, 1, 1), Z(i32, 1, 2), Z(i32, 1, N)]

    def check(what, call, outs):
        for o in outs:
            o.fill_(-7)
        rc = call(*[P(o) for o in outs])
        torch.cuda.synchronize()
        msg = _lib.load().gl_last_error_string().decode()
        assert rc != 0 and "capacity" in msg, (what, rc, msg)
        assert all(bool((o == -7).all()) for o in outs), what

    for NF, NP in ((3073, 16), (16, 4097)):
        out = [torch.empty((1, NF), dtype=i32, device="cuda"), torch.empty(1, dtype=i32, device="cuda")]
        a = [P(t) for t in feats(NF) + [Z(u8, 1, NF), Z(f64, 1, NP, 3), Z(i32, 1, NP), Z(f64, 1, NP), Z(u8, 1, NP), Z(u8, 1, NP, 32)]]
        check(("projection", NF, NP), lambda m, n: lib.gl_search_by_projection(ctx.h, C.byref(cam), 1.2, 1, NF, NP, *a, 3.0, 0.8, m, n), out)
        fe = feats(NF)
        a = [P(t) for t in [Z(f64, 1, 7), Z(f64, 1, 7)] + fe[:3] + [Z(f32, 1, NF), fe[3], Z(u8, 1, NF), Z(f64, 1, NP, 3), Z(u8, 1, NP), Z(i32, 1, NP),
                                                                  Z(f32, 1, NP), Z(u8, 1, NP, 32)]]
        check(("last frame", NF, NP), lambda m, n: lib.gl_search_by_projection_frame(ctx.h, C.byref(cam), 1.2, 1, NF, NP, *a, 7.0, 0, 1, m, n), out)
    for N1, N2 in ((4097, 16), (16, 4097)):
        a1, a2 = [P(t) for t in kf(N1, True)], [P(t) for t in kf(N2, True)]
        fm, ep = P(Z(f64, 1, 9)), P(Z(f32, 1, 2))
        check(("triangulation", N1, N2), lambda m, n: lib.gl_search_for_triangulation(ctx.h, 1.2, 1, N1, N2, 1, 1, *a1, *a2, fm, ep, 0, 1, m, n),
              [torch.empty((1, N1), dtype=i32, device="cuda"), torch.empty(1, dtype=i32, device="cuda")])
        b1, b2 = [P(t) for t in kf(N1, False)], [P(t) for t in kf(N2, False)]
        del b2[2]  # (the frame has no map-point flags)
        check(("bow", N1, N2), lambda m, n: lib.gl_search_by_bow(ctx.h, 0.7, 1, 1, N1, N2, 1, 1, *b1, *b2, m, n),
              [torch.empty((1, N2), dtype=i32, device="cuda"), torch.empty(1, dtype=i32, device="cuda")])
    NF, NP = 16385, 16
    a = [P(t) for t in feats(NF) + [Z(f64, 1, NP, 3), Z(i32, 1, NP), Z(u8, 1, NP), Z(u8, 1, NP, 32)]]
    check(("fuse", NF), lambda bi, bd: lib.gl_fuse_search(ctx.h, C.byref(cam), 1.2, 1, NF, NP, *a, 3.0, bi, bd),
          [torch.empty((1, NP), dtype=i32, device="cuda"), torch.empty((1, NP), dtype=i32, device="cuda")])
