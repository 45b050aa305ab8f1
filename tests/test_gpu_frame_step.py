"""gl_track_frame_end, gl_map_note_replaced and gl_track_frame_next on the device against the sequential model of
tests/frame_step_ref.py, the restatement of tests/frame_step_glue.py and the declared outputs of tests/frame_step_cases.py: every
integer, flag and row and the bits of ratio_map exactly; the four poses within a derived bound; and frame_step.track_frame_step over a
sequence of frames against the route through the host.  The expected output always comes from the model or the declaration, never from
the device.

THE POSE BOUND.  t_rc, t_cr, pose_lw and pose_cw are at most three chained SE3Quat products and two inverses behind the inputs, each
with its normalisation: well under a hundred fp64 operations on magnitudes of at most about 10 m, each rounding within 1.1e-16
relative, so below 1e-13 absolute - against the same statements evaluated in np.longdouble.  The tests hold 1e-12 * max(1, |t|): a
factor of ten above what the arithmetic can lose, far below anything a wrong operand order or a missing normalisation would give."""
import functools

import numpy as np
import pytest

from gmmloc_amd import api, frame_step, key_frame, map_stats
from tests import frame_step_cases as FC
from tests import frame_step_glue as G
from tests import frame_step_ref as R
from tests import frame_step_scenes as S
from tests.chain_glue import TH_LOCAL, TH_MM
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.gpu_helpers import stop_on_device_error, to_dev  # noqa: F401 (the fixture is autouse)
from tests.test_frame_step_cases import check_end_case, check_next_rows, next_args, poison_end, pose_bound

pytestmark = pytest.mark.gpu
F32 = np.float32
MAP_KEYS = ("mp_valid", "obs_ptr", "obs_kf", "kf_valid", "kf_mp", "mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc")
BA_KEYS = ("kf_pose", "kf_uvr", "kf_oct", "obs_feat")
POSES = ("t_rc", "t_cr", "pose_lw", "pose_cw")
RULE = dict(num_kfs=3, frame_idx=100, kf_frame_idx=90, fps=20.0, is_idle=1, n_queue=0)


def host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def map_dev(torch, m, ba):
    return to_dev(torch, m, MAP_KEYS), dict(to_dev(torch, ba, BA_KEYS), kf_first=int(ba.get("kf_first", -1)))


def device_end(torch, ctx, md, bd, a, th_depth, rule=None, poison=None):
    d = to_dev(torch, a)
    chain = {k: d.get(k) for k in ("feat_mp", "match_last", "match_local", "outlier", "counts2")}
    lm = {k: d.get(k) for k in ("local_mp", "n_local_mp", "ref_kf")}
    out = None if poison is None else to_dev(torch, poison)
    def call(torch, c):
        r = frame_step.frame_end(c, md, bd, chain, lm, d["feat_depth"], th_depth, last_observed=d.get("last_observed"),
                                 rule=None if rule is None else frame_step.kf_rule(**rule), out=out)
        torch.cuda.synchronize()
        return host(r)
    return run(call, torch, ctx)


def device_next(torch, ctx, md, bd, pose_tracked, pose_prev, ref_kf, held_mp, feat_new=None, mp_base=0, mp_replaced=None, poison=None, want_desc=True):
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = None if poison is None else to_dev(torch, poison)
    def call(torch, c):
        r = frame_step.frame_next(c, md, bd, T(pose_tracked), T(pose_prev), T(ref_kf), T(np.asarray(held_mp, np.int32)), feat_new=T(feat_new),
                                  mp_base=mp_base, mp_replaced=T(mp_replaced), want_desc=want_desc, out=out)
        torch.cuda.synchronize()
        return host(r)
    return run(call, torch, ctx)


def same_bytes(a, b, keys=None, what=""):
    for k in (a if keys is None else keys):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


# ---- the hand-built cases

def test_end_case(gpu):
    torch, ctx = gpu
    m, ba = FC.small_map()
    md, bd = map_dev(torch, m, ba)
    a = FC.end_arrays()
    out = device_end(torch, ctx, md, bd, a, FC.TH_DEPTH, FC.END_RULE, poison_end(4, len(FC.END)))
    check_end_case(out)
    same_bytes(out, R.frame_end(m, ba, th_depth=FC.TH_DEPTH, rule=FC.END_RULE, poison=poison_end(4, len(FC.END)), **a), ("held_mp", "held", "stat", "ratio_map"))
    # without last_observed and counts2: every frame tracked, no output changes
    b = dict(a, last_observed=None, counts2=None)
    out = device_end(torch, ctx, md, bd, b, FC.TH_DEPTH)
    assert out["stat"][:3].tolist() == [[1, 9, 4, 8, 0, 0, 0, 0]] * 3 and out["held_mp"][1].tolist() == FC.END_HELD_MP


@pytest.mark.parametrize("key", list(FC.COUNT))
def test_count_map_points(gpu, key):
    torch, ctx = gpu
    num_kfs, ref_kf = key
    m, ba = FC.small_map()
    md, bd = map_dev(torch, m, ba)
    a = FC.end_arrays()
    a["ref_kf"][:] = ref_kf
    out = device_end(torch, ctx, md, bd, a, FC.TH_DEPTH, dict(FC.END_RULE, num_kfs=num_kfs))
    assert out["stat"][[0, 2, 3], 4].tolist() == [FC.COUNT[key]] * 3 and out["stat"][1, 4] == 0


@functools.lru_cache(maxsize=None)
def rule_map_dev():
    import torch
    return map_dev(torch, *FC.rule_map())


@pytest.mark.parametrize("name", list(FC.RULES))
def test_need_new_keyframe_at_its_thresholds(gpu, name):
    torch, ctx = gpu
    _, nmi, num_map, num_total, nref, verdict = FC.RULES[name]
    md, bd = rule_map_dev()
    out = device_end(torch, ctx, md, bd, FC.rule_frame(nmi, num_map, num_total), FC.TH_DEPTH, FC.rule_of(name))
    assert out["stat"][0].tolist() == [1, nmi, num_map, num_total, nref, verdict, 0, 0], name
    assert out["ratio_map"][0].tobytes() == (F32(num_map) / F32(max(1, num_total))).tobytes()


def device_note(torch, ctx, rep, src, tgt, n=None, count=None):
    T = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    full = T(np.concatenate([rep, np.full(8, -9, np.int32)]))  # guard words behind the table
    def call(torch, c):
        frame_step.note_replaced(c, full[:len(rep)], T(src), T(tgt), n=n, n_dev=None if count is None else T([count]))
        torch.cuda.synchronize()
        return full.cpu().numpy()
    out = run(call, torch, ctx)
    assert (out[len(rep):] == -9).all(), "written behind mp_replaced"
    return out[:len(rep)]


@pytest.mark.parametrize("name", list(FC.REPLACE))
def test_note_replaced_cases(gpu, name):
    """`none`: an empty list (n = 0 on empty tensors) changes nothing"""
    torch, ctx = gpu
    steps, _ = FC.REPLACE[name]
    src, tgt = [s for s, _ in steps], [t for _, t in steps]
    none = -np.ones(FC.NMPCAP, np.int32)
    assert np.array_equal(device_note(torch, ctx, none, src, tgt), FC.replaced_array(name))
    old = np.arange(FC.NMPCAP, dtype=np.int32)[::-1].copy()
    for count in (0, 1, len(steps) + 3):  # the device count cuts the list and is clamped to it
        assert np.array_equal(device_note(torch, ctx, old, src + [0, 0, 0], tgt + [1, 1, 1], n=len(steps), count=count),
                              R.note_replaced(old, src, tgt, count)), (name, count)


@pytest.mark.parametrize("n", [1, 63, 65, 1023, 1024, 1025, 2500])
def test_note_replaced_long_lists(gpu, n):
    """random steps over few rows: sources repeat inside a chunk of 1 024 steps and across chunks, a tenth of the steps changes nothing"""
    torch, ctx = gpu
    rng = np.random.default_rng(300 + n)
    rows = 97
    src, tgt = rng.integers(-2, rows + 2, n), rng.integers(-2, rows + 2, n)
    same = rng.uniform(size=n) < 0.05
    tgt[same] = src[same]
    old = rng.integers(-1, rows, rows).astype(np.int32)
    want = R.note_replaced(old, src, tgt)
    assert np.array_equal(G.note_replaced(old, src, tgt), want)
    assert np.array_equal(device_note(torch, ctx, old, src, tgt), want)


def test_next_rows_case(gpu):
    torch, ctx = gpu
    m, ba, tracked, prev, ref_kf, held = next_args()
    md, bd = map_dev(torch, m, ba)
    rep = FC.replaced_array("all")
    fn = np.array([FC.NEXT_FEAT_NEW] * 2, np.int32)
    one = device_next(torch, ctx, md, bd, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep)
    check_next_rows(m, one, FC.NEXT_OUT)
    two = device_next(torch, ctx, md, bd, tracked, prev, ref_kf, one["held_mp"], mp_replaced=rep)  # A -> B -> C: B this frame, C the next
    check_next_rows(m, two, FC.NEXT_OUT_2)
    plain = device_next(torch, ctx, md, bd, tracked, prev, ref_kf, held)
    check_next_rows(m, plain, FC.NEXT_PLAIN)
    assert (one["status"] == 0).all()
    ref = R.frame_next(m, ba, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep)
    same_bytes(ref, one, ("held_mp", "last_pt", "last_valid", "last_observed", "held", "status"))
    # the rows' descriptors are the map points'; a slot without a row keeps its bytes
    poison = dict(last_desc=np.full((2, len(FC.NEXT_HELD), 32), 0x5a, np.uint8))
    full = G.frame_next(m, ba, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep, poison=poison)
    z = lambda *s, dt=np.float64: np.zeros(s, dt)
    B, NF = held.shape
    outs = dict(t_rc=z(B, 7), t_cr=z(B, 7), pose_lw=z(B, 7), pose_cw=z(B, 7), last_pt=z(B, NF, 3), last_valid=z(B, NF, dt=np.uint8),
                last_observed=z(B, NF, dt=np.uint8), held=z(B, NF, dt=np.uint8), status=z(B, dt=np.int32), last_desc=poison["last_desc"])
    got = device_next(torch, ctx, md, bd, tracked, prev, ref_kf, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep, poison=outs)
    assert got["last_desc"].tobytes() == full["last_desc"].tobytes() and (got["last_desc"][0, 6] == 0x5a).all()


def test_next_rows_then_temporal_points_case(gpu):
    """gl_create_temporal_points on the rows gl_track_frame_next wrote, held_mp passed as last_mp: a walked held == 2 slot - the invalid
    row one step of mp_replaced led to, a valid row without observations - ends with last_mp = -1, an unwalked one keeps its row"""
    torch, ctx = gpu
    m, ba, tracked, prev, ref_kf, held = next_args()
    md, bd = map_dev(torch, m, ba)
    rep = FC.replaced_array("all")
    fn = np.array([FC.NEXT_FEAT_NEW] * 2, np.int32)
    depth = np.array([FC.NEXT_DEPTH] * 2, F32)
    B, NF = held.shape
    rng = np.random.default_rng(4)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fr = dict(feat_uv=T(rng.uniform(20, 300, (B, NF, 2))), feat_depth=T(depth), feat_oct=T(np.zeros((B, NF), np.int32)),
              last_outlier=T(np.zeros((B, NF), np.uint8)), feat_desc=T(rng.integers(0, 256, (B, NF, 32), dtype=np.uint8)))
    def call(torch, c):
        nxt = frame_step.frame_next(c, md, bd, T(tracked), T(prev), T(ref_kf), T(held), feat_new=T(fn), mp_base=FC.NEXT_MP_BASE, mp_replaced=T(rep), want_desc=True)
        rows = nxt["held_mp"].clone()
        tmp = key_frame.create_temporal_points(c, api.Camera(), dict(fr, pose=nxt["pose_lw"], held=nxt["held"]),
                                               {k: nxt[k] for k in ("last_pt", "last_observed", "last_valid", "last_desc")}, FC.TH_DEPTH, last_mp=nxt["held_mp"])
        torch.cuda.synchronize()
        return host(dict(rows=rows, held=nxt["held"], last_mp=nxt["held_mp"], temp_flag=tmp["temp_flag"], last_observed=nxt["last_observed"]))
    out = run(call, torch, ctx)
    flag, last_mp = G.temporal_last_mp(out["rows"], out["held"], depth, FC.TH_DEPTH)
    for b in range(B):
        assert out["rows"][b].tolist() == FC.NEXT_OUT["held_mp"] and out["held"][b].tolist() == FC.NEXT_OUT["held"]
        assert out["temp_flag"][b].tolist() == flag[b].tolist() == FC.NEXT_TEMPORAL["temp_flag"]
        assert out["last_mp"][b].tolist() == last_mp[b].tolist() == FC.NEXT_TEMPORAL["last_mp"]
        assert (out["last_observed"][b][np.array(FC.NEXT_TEMPORAL["temp_flag"]) == 1] == 0).all()


def test_next_poses_case(gpu):
    """pose_prev NULL against given, a reference key-frame moved by a BA between end and next, a ref_kf outside the table"""
    torch, ctx = gpu
    m, ba, tracked, prev, ref_kf, held = next_args()
    md, bd = map_dev(torch, m, ba)
    LD = np.longdouble
    for pp in (None, prev):
        ref = R.frame_next(m, ba, tracked.astype(LD), None if pp is None else pp.astype(LD), ref_kf, held, dtype=LD)
        out = device_next(torch, ctx, md, bd, tracked, pp, ref_kf, held)
        for b in range(2):
            for k in POSES:
                assert np.abs(out[k][b] - ref[k][b]).max() <= pose_bound(ref[k][b]), (k, b)
            if pp is None:
                assert out["pose_cw"][b].tobytes() == out["pose_lw"][b].tobytes()
            else:
                assert np.abs(out["pose_cw"][b] - out["pose_lw"][b]).max() > 1e-3
    moved = dict(ba, kf_pose=ba["kf_pose"].copy())
    moved["kf_pose"][1, 4:] += [0.01, -0.02, 0.03]
    md2, bd2 = map_dev(torch, m, moved)
    a, b2 = device_next(torch, ctx, md, bd, tracked, prev, ref_kf, held), device_next(torch, ctx, md2, bd2, tracked, prev, ref_kf, held)
    ref2 = R.frame_next(m, moved, tracked.astype(LD), prev.astype(LD), ref_kf, held, dtype=LD)
    assert np.abs(a["t_rc"][0] - b2["t_rc"][0]).max() > 1e-3 and a["t_rc"][1].tobytes() == b2["t_rc"][1].tobytes()
    for k in POSES:
        assert np.abs(b2[k][0] - ref2[k][0]).max() <= pose_bound(ref2[k][0]), k
    poison = {k: np.full((2, 7), -77.0) for k in POSES}
    for bad in (-1, FC.NKF):
        z = lambda *s, dt=np.float64: np.zeros(s, dt)
        outs = dict(poison, last_pt=z(2, 10, 3), last_valid=z(2, 10, dt=np.uint8), last_observed=z(2, 10, dt=np.uint8), held=z(2, 10, dt=np.uint8),
                    status=np.full(2, -77, np.int32))
        out = device_next(torch, ctx, md, bd, tracked, prev, np.array([bad, 0], np.int32), held, poison=outs, want_desc=False)
        assert out["status"].tolist() == [R.BAD_REF, 0]
        assert all((out[k][0] == -77.0).all() and (out[k][1] != -77.0).all() for k in POSES)
        check_next_rows(m, out, FC.NEXT_PLAIN)


# ---- malformed rows: every access they would make lies inside a live allocation of the test (the tables are views into padded buffers)

PAD = 64


def padded(torch, a, fill):
    a = np.ascontiguousarray(a)
    per = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    full = np.concatenate([np.full(PAD * per, fill, a.dtype), a.ravel(), np.full(PAD * per, fill, a.dtype)])
    t = torch.from_numpy(full).cuda()
    return t, t[PAD * per:PAD * per + a.size].view(*a.shape)


def test_malformed_rows_change_nothing_and_fault_nothing(gpu):
    """rows up to PAD entries outside their tables in feat_mp, local_mp, held_mp, feat_new and mp_replaced, CSR ranges outside [0, NOBS]:
    skipped as the restatement says, the padding keeps its bytes"""
    torch, ctx = gpu
    m, ba = (dict(d) for d in S.random_map())
    NMP, NOBS = len(m["obs_ptr"]) - 1, len(m["obs_kf"])
    rng = np.random.default_rng(71)
    m["obs_ptr"] = m["obs_ptr"].copy()
    m["obs_ptr"][rng.choice(NMP, 20, replace=False)] = rng.choice(np.array([-1, -5, NOBS + 1, NOBS + 9]), 20)
    fills = {"mp_valid": 1, "obs_ptr": 0, "obs_kf": 0, "kf_valid": 1, "kf_mp": -1, "mp_pos": 7.0, "mp_desc": 0x33}
    keep, md = {}, {}
    for k, fill in fills.items():
        keep[k], md[k] = padded(torch, m[k], fill)
    for k in ("mp_normal", "mp_max_dist", "mp_min_dist"):
        md[k] = torch.from_numpy(m[k]).cuda()
    bd = dict(to_dev(torch, ba, BA_KEYS), kf_first=0)
    bad = lambda shape: rng.choice(np.concatenate([np.arange(NMP, NMP + PAD // 2), np.arange(-PAD // 2, -1)]), shape).astype(np.int32)
    B, NF = 2, 65
    a = S.random_end(m, B, NF, 72)
    at = rng.uniform(size=(B, NF)) < 0.3
    a["feat_mp"][at] = bad(int(at.sum()))
    at = rng.uniform(size=a["local_mp"].shape) < 0.3
    a["local_mp"][at] = bad(int(at.sum()))
    a["n_local_mp"][:] = [a["local_mp"].shape[1] + 5, -3]  # clamped to [0, NPcap]
    a["ref_kf"][:] = [m["kf_mp"].shape[0], 3]
    a["counts2"][:, 3] = 0
    out = device_end(torch, ctx, md, bd, a, S.TH_DEPTH, RULE)
    same_bytes(G.frame_end(m, ba, th_depth=S.TH_DEPTH, rule=RULE, **a), out, what="end")
    n = S.random_next(m, B, NF, 73, NMPcap=NMP + PAD // 2)
    at = rng.uniform(size=(B, NF)) < 0.3
    n["held_mp"][at] = bad(int(at.sum()))
    n["feat_new"][rng.uniform(size=(B, NF)) < 0.1] = NMP  # (mp_base + NMP: far outside, compared in 64 bits)
    at = rng.uniform(size=len(n["mp_replaced"])) < 0.3
    n["mp_replaced"][at] = bad(int(at.sum()))
    n["ref_kf"][:] = [2, -4]
    want = G.frame_next(m, ba, **n)
    got = device_next(torch, ctx, md, bd, **n)
    same_bytes(want, got, ("held_mp", "last_pt", "last_valid", "last_observed", "held", "status", "last_desc"), "next")
    assert got["status"].tolist() == [0, R.BAD_REF]
    for k, fill in fills.items():
        full = keep[k].cpu().numpy()
        per = full.size // (2 * PAD + len(m[k])) if len(m[k]) else 1
        assert (full[:PAD * per] == fill).all() and (full[-PAD * per:] == fill).all(), k
    src = np.concatenate([bad(40), rng.integers(0, NMP, 40)]).astype(np.int32)
    tgt = np.concatenate([rng.integers(0, NMP, 40), bad(40)]).astype(np.int32)
    old = rng.integers(-1, NMP, NMP).astype(np.int32)
    assert np.array_equal(device_note(torch, ctx, old, src, tgt), old)


# ---- random frames across a lane, a wave and a workgroup edge, and at the bound

SHAPES = [(B, NF) for NF in (1, 63, 65, 257) for B in (1, 3)] + [(1, 3072)]


@pytest.mark.parametrize("B,NF", SHAPES)
def test_end_random(gpu, B, NF):
    """against the model, exactly; alone against in a batch and on a second call on the used context, bit for bit"""
    torch, ctx = gpu
    m, ba = S.random_map()
    md, bd = map_dev(torch, m, ba)
    a = S.random_end(m, B, NF, 500 + NF)
    W = R.World(m, ba)
    ref = R.frame_end(m, ba, th_depth=S.TH_DEPTH, rule=RULE, world=W, **a)
    assert ref["is_outlier"].tobytes() == a["outlier"].tobytes()
    if NF >= 63:
        for k in ("inlier", "outlier_row", "cleared_row", "matched_local", "from_last", "temporal"):
            assert W.events[k] > 0, k
    out = device_end(torch, ctx, md, bd, a, S.TH_DEPTH, RULE)
    same_bytes(out, ref, ("held_mp", "held", "stat", "ratio_map"), "model")
    same_bytes(out, G.frame_end(m, ba, th_depth=S.TH_DEPTH, rule=RULE, **a), what="glue")
    same_bytes(out, device_end(torch, ctx, md, bd, a, S.TH_DEPTH, RULE), what="second call")
    for b in range(B):
        one = {k: (v[b:b + 1] if v is not None else None) for k, v in a.items()}
        alone = device_end(torch, ctx, md, bd, one, S.TH_DEPTH, RULE)
        same_bytes({k: v[b:b + 1] for k, v in out.items()}, alone, what="alone %d" % b)


@pytest.mark.parametrize("B,NF", SHAPES)
def test_next_random(gpu, B, NF):
    torch, ctx = gpu
    m, ba = S.random_map()
    md, bd = map_dev(torch, m, ba)
    n = S.random_next(m, B, NF, 600 + NF)
    LD = np.longdouble
    W = R.World(m, ba, LD)
    ref = R.frame_next(m, ba, **dict(n, pose_tracked=n["pose_tracked"].astype(LD), pose_prev=n["pose_prev"].astype(LD)), dtype=LD, world=W)
    if NF >= 63:
        for k in ("stereo_new", "stereo_nulled", "replaced", "held_unobserved"):
            assert W.events[k] > 0, k
    out = device_next(torch, ctx, md, bd, **n)
    same_bytes(ref, out, ("held_mp", "last_pt", "last_valid", "last_observed", "held", "status"), "model")
    same_bytes(G.frame_next(m, ba, **n), out, ("held_mp", "last_pt", "last_valid", "last_observed", "held", "status", "last_desc"), "glue")
    for b in range(B):
        for k in POSES:
            assert np.abs(out[k][b] - ref[k][b]).max() <= pose_bound(ref[k][b]), (k, b)
    same_bytes(out, device_next(torch, ctx, md, bd, **n), what="second call")
    for b in range(B):
        one = {k: (v[b:b + 1] if k in ("pose_tracked", "pose_prev", "ref_kf", "held_mp", "feat_new") else v) for k, v in n.items()}
        alone = device_next(torch, ctx, md, bd, **one)
        same_bytes({k: v[b:b + 1] for k, v in out.items()}, alone, what="alone %d" % b)


# ---- the sequence: T consecutive frames, the device hand-over against the route through the host

CHAIN_OUT = ("pose", "pose_mm", "match_last", "match_local", "outlier", "counts", "inview", "drop_src", "counts2", "feat_mp")
LIST_KEYS = ("local_kf", "n_local_kf", "local_mp", "n_local_mp", "ref_kf", "status")
LAST_KEYS = ("last_pt", "last_valid", "last_observed", "last_desc")
KW = dict(th_mm=TH_MM, th_local=TH_LOCAL, nn_ratio=0.8)
GROW = dict(mp=400, obs=2000, kf=1)  # spare rows behind the sequence's map: what a key-frame pass may add


class Resident:
    """a fresh upload of the sequence's map into capacity buffers (map_grow's module docstring), its counters, lists and first state"""

    def __init__(self, torch, q):
        from gmmloc_amd import map_grow
        self.torch, self.grow = torch, map_grow
        m, ba = q["s"]["map"], q["ba"]
        NMP, (NKF, NFK), NOBS = len(m["mp_valid"]), m["kf_mp"].shape, len(m["obs_kf"])
        lead = {"obs_kf": GROW["obs"], "obs_feat": GROW["obs"], "kf_valid": GROW["kf"], "kf_mp": GROW["kf"], "kf_pose": GROW["kf"], "kf_uvr": GROW["kf"],
                "kf_oct": GROW["kf"]}
        fill = {"kf_mp": -1}
        def cap(k, a):
            a = np.ascontiguousarray(a)
            extra = np.full((lead.get(k, GROW["mp"]),) + a.shape[1:], fill.get(k, 0), a.dtype)
            return torch.from_numpy(np.concatenate([a, extra])).cuda()
        self.md = {k: cap(k, m[k]) for k in MAP_KEYS}
        self.bd = {k: cap(k, ba[k]) for k in BA_KEYS}
        self.bd["mp_assoc"] = torch.full((NMP + GROW["mp"],), -1, dtype=torch.int32).cuda()
        self.bd["kf_first"] = 0
        self.sizes = (NMP, NKF, NOBS)
        self.st = map_stats.map_stats_alloc(NMP + GROW["mp"], 8)
        self.st["visible"][:NMP] = 1
        self.st["found"][:NMP] = 1
        self.mp_replaced = torch.full((NMP + GROW["mp"],), -1, dtype=torch.int32).cuda()
        first = to_dev(torch, {k: np.asarray(v)[None] for k, v in q["first"].items()})
        # (without the optional kf_count: its row follows NKF, which a key-frame pass changes)
        self.state = frame_step.first_state(first, first["last_mp"], to_dev(torch, {k: v for k, v in q["lists"].items() if k != "kf_count"}))

    def views(self):
        md, bd = self.grow.map_views(self.md, self.bd, self.sizes)
        return md, {k: v for k, v in bd.items() if k != "mp_assoc"}

    def mirror(self):
        """the host's copy of the map as it is now"""
        md, bd = self.views()
        return host(md), host(bd)


def fuse_pass(ctx, M, q, begun, frame, extra):
    """a mapping pass that has finished while the frame was tracked: fuse matches of key-frame 0 that replace points of the frame's local
    map (candidates and slots fixed by the scene, not by the tracker), ptr_replaced_ and the counters kept beside it; then map_remove
    culls up to eight targets that took over a row the frame holds.  -> the keyword arguments of track_frame_finish"""
    torch = M.torch
    m = q["s"]["map"]
    k = int(np.nonzero(m["kf_valid"])[0][0])
    slots = np.nonzero((m["kf_mp"][k] >= 0) & (m["mp_valid"][np.maximum(m["kf_mp"][k], 0)] != 0))[0]
    seen_by_k = set(m["kf_mp"][k][m["kf_mp"][k] >= 0].tolist())
    cand = [int(p) for p in q["s"]["rows"][0] if m["mp_valid"][p] and p not in seen_by_k and m["obs_ptr"][p + 1] > m["obs_ptr"][p]][:min(len(slots), 150)]
    T = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    r = M.grow.map_fuse(ctx, M.md, M.bd, k, T(cand), T(slots[:len(cand)]), sizes=M.sizes)
    assert r["status"] == 0 and r["n_replaced"] >= 20, (r["status"], r["n_replaced"])
    M.sizes = r["sizes"]
    map_stats.map_stats_merge(ctx, M.st, M.sizes[0], r["repl_src"], r["repl_tgt"])
    frame_step.note_replaced(ctx, M.mp_replaced, r["repl_src"], r["repl_tgt"])
    extra.update(repl_src=r["repl_src"].cpu().numpy(), repl_tgt=r["repl_tgt"].cpu().numpy(), mp_replaced=M.mp_replaced.cpu().numpy())
    # ... and a cull behind it: targets that took over a row the frame holds are removed, so that ONE step of mp_replaced leads the frame
    # to an invalid, empty row (held == 2), which createTemporalPoints then replaces
    held = begun["end"]["held_mp"][0].cpu().numpy()
    victims = np.unique(extra["repl_tgt"][np.isin(extra["repl_src"], held[held >= 0])])[:8]
    assert len(victims) >= 1, "no held row of the frame was replaced"
    md, bd = M.views()
    rm = api.map_remove(ctx, md, bd, rm_mp=T(victims))
    assert rm["status"] == 0 and rm["n_dead"] >= len(victims), (rm["status"], rm["n_dead"])
    M.sizes = (M.sizes[0], M.sizes[1], rm["nobs"])
    extra.update(victims=victims)
    return dict(mp_replaced=M.mp_replaced)


def stereo_pass(ctx, M, q, begun, frame, extra):
    """the frame becomes key-frame row NKF: its table rows, createMapPointsFromStereo (no GMM candidates: FromDepth), the new rows and
    their observations into the map, the walk of processNewKeyFrame, the new rows' counters; ref_kf becomes the new row"""
    torch = M.torch
    cam, prm = q["cam"], api.Params()
    NMP, NKF, NOBS = M.sizes
    B, NF = frame["feat_oct"].shape
    M.md["kf_mp"][NKF].copy_(begun["end"]["held_mp"][0])
    M.bd["kf_uvr"][NKF].copy_(torch.cat([frame["feat_uv"][0], frame["feat_ur"][0].double()[:, None]], 1))
    M.bd["kf_oct"][NKF].copy_(frame["feat_oct"][0])
    M.bd["kf_pose"][NKF].copy_(begun["chain"]["pose"][0])
    if "gmm" not in extra:
        from gmmloc_amd import synth
        extra["gmm"] = api.GMM(ctx, *synth.synth_gmm(64, 3))
    row = torch.full((1,), NKF, dtype=torch.int32).cuda()
    z = lambda *s: torch.zeros(s, dtype=torch.int32).cuda()
    sp = key_frame.create_stereo_points(ctx, extra["gmm"], cam, prm, dict(pose=begun["chain"]["pose"], feat_uv=frame["feat_uv"], feat_ur=frame["feat_ur"],
                                                                         feat_depth=frame["feat_depth"], feat_oct=frame["feat_oct"], cand=z(B, NF, 1),
                                                                         ncand=z(B, NF), held=begun["end"]["held"], kf_row=row), NMP, True, S.TH_DEPTH)
    r = M.grow.map_add(ctx, M.md, M.bd, sizes=(NMP, NKF + 1, NOBS), new_mp=dict(pos=sp["new_pos"][0], assoc=sp["new_assoc"][0]), new_kf=row,
                       attach=dict(mp=sp["att_mp"][0], kf=sp["att_kf"][0], feat=sp["att_feat"][0]), walk_kf=row, n_new_mp=sp["n_new"], n_attach=sp["n_new"])
    assert r["status"] == 0 and r["sizes"][0] - NMP >= 20 and r["n_attached"] >= 20, (r["status"], r["sizes"], r["n_attached"])
    M.sizes = r["sizes"]
    n = M.sizes[0] - NMP  # (the new rows' descriptor: the feature's own - one observation each, what computeDistinctiveDescriptors gives)
    M.md["mp_desc"][NMP:NMP + n] = frame["feat_desc"][0][sp["new_feat"][0, :n].long()]
    map_stats.map_stats_new_points(ctx, M.st, NKF + 1, NMP, sp["new_ref_kf"][0], n_dev=sp["n_new"])
    begun["lm"]["ref_kf"].fill_(NKF)  # (gmmloc_opt.cpp:27)
    extra.update(feat_new=sp["feat_new"].cpu().numpy(), mp_base=NMP, n_new=r["sizes"][0] - NMP)
    return dict(feat_new=sp["feat_new"], mp_base=NMP, is_key_frame=True)


def keep_frame(begun, r, state):
    """device tensors of one frame to compare afterwards; the in/out buffers that later frames write are cloned ON the device"""
    return dict({k: begun["chain"][k] for k in CHAIN_OUT}, **{k: v.clone() for k, v in state["lists"].items()},
                stat=begun["end"]["stat"], ratio_map=begun["end"]["ratio_map"], held_mp=r["next"]["held_mp"], pose_lw=r["next"]["pose_lw"],
                pose_cw=r["next"]["pose_cw"], t_rc=r["next"]["t_rc"], held=r["next"]["held"], n_temp=None if r["temporal"] is None else r["temporal"]["n_temp"],
                temp_flag=None if r["temporal"] is None else r["temporal"]["temp_flag"],
                **{k: state[k].clone() for k in LAST_KEYS})


def device_leg(torch, ctx, q, between=None):
    """frame after frame on the device, nothing read back between two frames (a key-frame pass reads its own few bytes) -> per frame the
    host copies, taken after the last frame"""
    cam, prm = q["cam"], api.Params()
    M = Resident(torch, q)
    extra = {}
    fds = [frame_dev(torch, f) for f in q["frames"]]  # (every frame's features are on the device before the first call)
    def call(torch, c):
        state, kept = M.state, []
        for t, fd in enumerate(fds):
            rule = frame_step.kf_rule(**dict(RULE, frame_idx=100 + t))
            md, bd = M.views()
            if between is not None and t == between[0]:
                begun = frame_step.track_frame_begin(c, cam, prm, state, fd, md, bd, M.st, S.TH_DEPTH, rule=rule, **KW)
                kw = between[1](c, M, q, begun, fd, extra)
                md, bd = M.views()
                state, r = frame_step.track_frame_finish(c, cam, state, fd, md, bd, begun, S.TH_DEPTH, **kw)
            else:
                state, r = frame_step.track_frame_step(c, cam, prm, state, fd, md, bd, M.st, S.TH_DEPTH, rule=rule, **KW)
                begun = r
            kept.append(keep_frame(begun, r, state))
        torch.cuda.synchronize()
        return kept
    kept = run(call, torch, ctx)
    return [host({k: v for k, v in f.items() if v is not None}) for f in kept], host({k: M.st[k] for k in ("visible", "found")}), extra


def frame_dev(torch, f):
    return to_dev(torch, {k: np.asarray(v)[None] for k, v in f.items()})


def features_depth(f):
    """the depths of the frame's FEATURES for the model: a slot of the device's arrays whose octave is outside 0 .. 7 is padding
    (gmmloc_hip.h), no feature of the reference's frame - depth 0 keeps it out of createTemporalPoints' list"""
    oct_ = np.asarray(f["feat_oct"])
    return np.where((oct_ >= 0) & (oct_ <= 7), np.asarray(f["feat_depth"], F32), F32(0)).astype(F32)


def host_leg(torch, ctx, q, between=None):
    """today's route: track_frame_chain_map (with its counters) -> copy back -> the model's hand-over on the host -> upload.  The poses
    of the hand-over are the DEVICE's (frame_step.frame_next on the uploaded rows), as tests/track_ref.py takes pose_mm: a last-ulp
    difference cannot move a window edge."""
    cam, prm = q["cam"], api.Params()
    M = Resident(torch, q)
    m, ba = q["s"]["map"], q["ba"]
    state, extra, frames = M.state, {}, []
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for t, f in enumerate(q["frames"]):
        fd = frame_dev(torch, f)
        md, bd = M.views()
        a = {k: fd[k] for k in frame_step.FRAME_KEYS if k != "feat_depth"}
        a.update({k: state[k] for k in frame_step.STATE_KEYS[:8] if state.get(k) is not None})
        lm = dict(state["lists"], last_mp=state["last_mp"])
        def chain(torch, c):
            out = map_stats.track_frame_with_stats(c, cam, prm, a, md, lm, M.st, **KW)
            torch.cuda.synchronize()
            return out
        out = run(chain, torch, ctx)
        h = dict(host({k: out[k] for k in CHAIN_OUT}), **host({k: lm[k] for k in LIST_KEYS if k in lm}))
        assert h["counts2"][0, 3] == 0, "frame %d was not tracked by the motion model" % t
        # the loop over the features, on the host: the model
        W = R.World(m, ba)
        last_observed = state["last_observed"].cpu().numpy() if state.get("last_observed") is not None else None
        end = R.frame_end(m, ba, h["feat_mp"], h["match_last"], h["match_local"], h["outlier"], h["local_mp"], h["n_local_mp"], h["counts2"], h["ref_kf"],
                          last_observed, f["feat_depth"][None], S.TH_DEPTH, rule=dict(RULE, frame_idx=100 + t), world=W)
        kw = {}
        if between is not None and t == between[0]:
            begun = dict(chain=out, end=to_dev(torch, {k: end[k] for k in ("held_mp", "held")}), lm=lm)
            def pass_(torch, c):
                r = between[1](c, M, q, begun, fd, extra)
                torch.cuda.synchronize()
                return r
            kw = run(pass_, torch, ctx)
            md, bd = M.views()
            m, ba = M.mirror()  # (the host's mirror of the map after the pass)
            h["ref_kf"] = lm["ref_kf"].cpu().numpy()
        pose_prev = None if state.get("first") else state["pose_lw"].cpu().numpy()
        rep = R.note_replaced(-np.ones(len(M.mp_replaced), np.int32), extra["repl_src"], extra["repl_tgt"]) if "mp_replaced" in kw else None
        assert rep is None or np.array_equal(rep, extra["mp_replaced"])  # (gl_map_note_replaced on the fuse's own lists)
        W2 = R.World(m, ba)
        made_key_frame = bool(kw.get("is_key_frame"))  # (a key-frame makes no temporal points, tracking.cpp:44: its rows stay)
        nxt = R.frame_next(m, ba, h["pose"], pose_prev, h["ref_kf"], end["held_mp"], feat_new=extra.get("feat_new") if "feat_new" in kw else None,
                           mp_base=kw.get("mp_base", 0), mp_replaced=rep, world=W2, feat_depth=None if made_key_frame else features_depth(f)[None],
                           th_depth=S.TH_DEPTH)
        last_mp = nxt["held_mp"] if made_key_frame else nxt["last_mp"]  # (mappoints_ as frame t + 1 finds them: the model's, not the device's)
        desc = np.where((nxt["held_mp"] >= 0)[..., None], m["mp_desc"][np.maximum(nxt["held_mp"], 0)], 0).astype(np.uint8)
        poses = device_next(torch, ctx, md, bd, h["pose"], pose_prev, h["ref_kf"], end["held_mp"], feat_new=extra.get("feat_new") if "feat_new" in kw else None,
                            mp_base=kw.get("mp_base", 0), mp_replaced=rep)
        for k in POSES:
            assert np.abs(poses[k][0] - nxt[k][0]).max() <= pose_bound(nxt[k][0]), (t, k)
        last = dict(last_pt=T(nxt["last_pt"]), last_observed=T(nxt["last_observed"]), last_valid=T(nxt["last_valid"]), last_desc=T(desc))
        pose_lw = T(poses["pose_lw"])
        n_temp = None
        if not made_key_frame:
            def temporal(torch, c):
                r = key_frame.create_temporal_points(c, cam, dict(pose=pose_lw, feat_uv=fd["feat_uv"], feat_depth=fd["feat_depth"], feat_oct=fd["feat_oct"],
                                                                  held=T(nxt["held"]), last_outlier=T(end["is_outlier"]), feat_desc=fd["feat_desc"]), last,
                                                     S.TH_DEPTH)
                torch.cuda.synchronize()
                return r
            n_temp = run(temporal, torch, ctx)["n_temp"].cpu().numpy()
            assert int(nxt["temp_flag"].sum()) == int(n_temp[0])  # (the model's walk and gl_create_temporal_points' own agree)
        h.update(host({k: v.clone() for k, v in state["lists"].items()}))
        h.update(stat=end["stat"], ratio_map=end["ratio_map"], held_mp=last_mp, held=nxt["held"], pose_lw=poses["pose_lw"], pose_cw=poses["pose_cw"],
                 t_rc=poses["t_rc"], **host(last))
        if n_temp is not None:
            h.update(n_temp=n_temp, temp_flag=nxt["temp_flag"])
        h["events"], h["events_next"] = W.events, W2.events
        frames.append(h)
        state = dict(last, pose_lw=pose_lw, pose_cw=T(poses["pose_cw"]), last_oct=fd["feat_oct"], last_angle=fd["feat_angle"], last_mp=T(last_mp),
                     lists=state["lists"], first=False)
    return frames, host({k: M.st[k] for k in ("visible", "found")}), extra


def compare_legs(q, dev_leg, host_leg_, key_frame_at=None):
    fd, sd, _ = dev_leg
    fh, sh, _ = host_leg_
    assert len(fd) == len(fh) == S.SEQ["T"]
    for t, (d, h) in enumerate(zip(fd, fh)):
        print("frame %d: counts %s counts2 %s stat %s ratio_map %s held rows %d temporal %s" % (t, d["counts"][0].tolist(), d["counts2"][0].tolist(),
              d["stat"][0].tolist(), d["ratio_map"][0], int((d["held_mp"] >= 0).sum()), d.get("n_temp")))
        assert ("n_temp" in d) == ("n_temp" in h) == (t != key_frame_at)
        for k in CHAIN_OUT + LIST_KEYS + LAST_KEYS + ("stat", "ratio_map", "held_mp", "held", "pose_lw", "pose_cw", "t_rc") + (("n_temp", "temp_flag") if "n_temp" in d else ()):
            assert d[k].tobytes() == h[k].tobytes(), (t, k)
        assert d["stat"][0, 0] == 1 and d["stat"][0, 1] >= 10 and d["counts2"][0, 3] == 0, (t, d["stat"], d["counts2"])
    same_bytes(sd, sh, what="counters")
    # the sequence is what it was built to be: rows and temporal points carried from frame to frame
    assert all(int((h["held_mp"] >= 0).sum()) >= 10 and int(h.get("n_temp", [10])[0]) >= 10 for h in fh)
    assert sum(h["events"]["temporal"] for h in fh[1:]) >= 10 and sum(h["events"]["matched_local"] for h in fh) >= 10
    assert (sd["visible"] > 1).sum() > 50 and (sd["found"] > 1).sum() > 20


def test_sequence_of_non_key_frames(gpu):
    torch, ctx = gpu
    q = S.sequence()
    compare_legs(q, device_leg(torch, ctx, q), host_leg(torch, ctx, q))


def test_sequence_with_a_fuse_pass_in_the_middle(gpu):
    """map_fuse + map_stats_merge + note_replaced, then a cull of some of the fuse's targets, between frame 2's end and its hand-over:
    frames 3 .. 5 run on the replaced rows, and on temporal points where the row a held one was replaced by is gone"""
    torch, ctx = gpu
    q = S.sequence()
    d, h = device_leg(torch, ctx, q, (2, fuse_pass)), host_leg(torch, ctx, q, (2, fuse_pass))
    compare_legs(q, d, h)
    assert np.array_equal(d[2]["mp_replaced"], h[2]["mp_replaced"]) and np.array_equal(d[2]["repl_src"], h[2]["repl_src"])
    assert h[0][2]["events_next"]["replaced"] >= 3, h[0][2]["events_next"]  # (held rows of the frame were among the replaced ones)
    plain = device_leg(torch, ctx, q)
    assert plain[0][2]["held_mp"].tobytes() != d[0][2]["held_mp"].tobytes()
    # a held row replaced onto a row that was culled behind the fuse: ONE step leads to an invalid, empty row (held == 2),
    # createTemporalPoints puts a temporal point there, last_mp is -1, and frame 3 keeps its match to that slot as a temporal one - a
    # last_mp that still named the culled row would make the chain drop the match as one to an invalid point
    e, f2, f3 = h[0][2]["events_next"], d[0][2], d[0][3]
    slots = np.nonzero((f2["held"][0] == 2) & (f2["temp_flag"][0] == 1))[0]
    kept = np.isin(slots, f3["match_last"][0])
    print("frame 2: culled targets %s, held == 2 slots made temporal %s, matched by frame 3: %d" % (d[2]["victims"].tolist(), slots.tolist(), int(kept.sum())))
    assert e["temporal_over_invalid_row"] >= 1 and len(slots) >= e["temporal_over_invalid_row"], e
    assert (f2["held_mp"][0][slots] == -1).all()
    assert kept.sum() >= 1, "frame 3 kept no match to a slot whose replaced row was made a temporal point"
    assert (f3["feat_mp"][0][np.isin(f3["match_last"][0], slots)] == -1).all()  # (held as temporal points: no row)


def test_sequence_with_a_key_frame_in_the_middle(gpu):
    """frame 2 becomes a key-frame: feat_new of create_stereo_points, the map grown by its points, ref_kf the new row"""
    torch, ctx = gpu
    q = S.sequence()
    d, h = device_leg(torch, ctx, q, (2, stereo_pass)), host_leg(torch, ctx, q, (2, stereo_pass))
    compare_legs(q, d, h, key_frame_at=2)
    assert np.array_equal(d[2]["feat_new"], h[2]["feat_new"]) and d[2]["n_new"] == h[2]["n_new"] >= 20
    NKF = q["s"]["map"]["kf_mp"].shape[0]
    assert h[0][2]["ref_kf"].tolist() == [NKF] and h[0][2]["events_next"]["stereo_new"] >= 20
    new = h[0][2]["held_mp"] >= d[2]["mp_base"]
    assert new.sum() >= 20 and (h[0][2]["last_observed"][new] == 1).all()  # (the new rows hold their observation by the new key-frame)
    assert (h[0][3]["feat_mp"] >= d[2]["mp_base"]).sum() >= 5, "frame 3 holds none of the key-frame's new points"
