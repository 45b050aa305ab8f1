"""A mapping session on the device: four consecutive key-frames through every step of Localization::spinOnce (tests/session_ref.py:
STEPS) on ONE set of capacity buffers and one context - nothing uploaded but each key-frame's own rows, nothing read back but what the
composites themselves read - against the model leg: every integer edit made on the host by the sequential models, the float producers
taken from the device on a map uploaded afresh before each of them.  The per-call tests start every step from a fresh upload; what only a
session can see - a step that reads rows an earlier one left stale, sizes threaded wrongly, a write just past the sizes that a later
growth exposes, a composite that omits a step - shows here as the first snapshot that differs.
The expected state always comes from the models, never from the device leg.  Scene, knobs and events: tests/session_scenes.py,
tests/test_session_ref.py."""
import numpy as np
import pytest

from gmmloc_amd import api, bow
from tests import session_ref as SR
from tests import session_scenes as SS
from tests.context_cases import close_context, new_context
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse)
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)

pytestmark = pytest.mark.gpu

POINT_KEYS = tuple(k for k, _, _ in SR.POINT_SPEC)
_cache = {}


@pytest.fixture(scope="module")
def world(gpu, map_v1, gt_sync):
    """the scene and the model leg, made once: (scene, the model leg's snapshots and results, its Host, its state on entry)"""
    torch, ctx = gpu
    mean, cov = map_v1
    cam = api.Camera()
    def make(torch, ctx):
        P = SR.DeviceProducers(torch, ctx, cam, mean, cov)
        sc = SS.session_scene(mean, cov, gt_sync["V1_01_easy"], P.search2d)
        out, H, entry = SR.model_leg(sc, P)
        return dict(sc=sc, model=out, H=H, entry=entry, cam=cam, gmm=P.gmm, voc=bow.Vocabulary.from_arrays(ctx, **sc["voc"]), mean=mean, cov=cov)
    return run(make, torch, ctx)


def generous_caps(w):
    need = w["H"].need
    return need["NMP"] + 300, need["NOBS"] + 3000, w["sc"]["NKF"], need["cand"] + 200


def leg(torch, ctx, w, caps, gmm=None, voc=None, **kw):
    """the device leg on fresh buffers of these capacities -> (per (K, step) the host's (snapshot, results), the Device)"""
    D = SR.Device(torch, ctx, w["sc"], w["entry"], caps, w["cam"], gmm or w["gmm"], voc or w["voc"])
    inputs = {K: w["model"][(K, SR.STEPS[0])][1]["inputs"] for K in w["sc"]["arrivals"]}
    def call(torch, ctx):
        out = SR.device_leg(D, inputs, **kw)
        torch.cuda.synchronize()
        return out
    out = run(call, torch, ctx)  # (every snapshot is a device clone: copied only now, after the last step)
    host = {key: (SR.snapshot_to_host(s), SR.results_to_host(key[1], r)) for key, (s, r) in out.items()}
    for what, t in D.status:
        assert not t.cpu().numpy().any(), ("status", what, t.cpu().numpy())
    D.guards_untouched()
    return host, D


def generous(gpu, w):
    if "generous" not in _cache:
        _cache["generous"] = leg(gpu[0], gpu[1], w, generous_caps(w))[0]
    return _cache["generous"]


def same_state(dev, ref, what, keys=None):
    assert sorted(dev) == sorted(ref), (what, sorted(dev), sorted(ref))
    alive = ref["mp_valid"] != 0
    for k in keys or sorted(ref):
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        if k in ("cov_kf", "cov_w") and a.shape[1] != b.shape[1]:  # (rows of another capacity: nothing was ever written behind the narrower one)
            W = min(a.shape[1], b.shape[1])
            assert not a[:, W:].any() and not b[:, W:].any(), (what, k, "an entry behind the narrower width")
            a, b = a[:, :W], b[:, :W]
        if k in POINT_KEYS and a.shape == b.shape:  # (update_map_points leaves the rows of an invalid point as they are)
            a, b = a[alive], b[alive]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            diff = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            raise AssertionError("key-frame %s, step %r, array %s: %d of %d elements differ, first at %s: %s != %s" %
                                 (what[0], what[1], k, len(diff), a.size, diff[0].tolist(), a[tuple(diff[0])], b[tuple(diff[0])]))


def test_session_equals_the_models_edits_uploaded(gpu, world):
    """after EVERY step of every key-frame, bit for bit: every map array cut to the sizes, obs_feat, mp_assoc, mp_ref_kf, kf_pose / kf_twc /
    mp_pos, the per-point arrays of the valid rows, visible / found / ref_idx, the candidate list, every table of the graph, mp_replaced,
    the BoW rows, and each step's own counts and lists.  (The replacement lists of the fuses inside search_in_neighbors_from_map are not
    among its results; mp_replaced, the counters and the map hold what they did.)"""
    dev = generous(gpu, world)
    ref = world["model"]
    assert list(dev) == list(ref)
    for key in ref:
        same_state(dev[key][0], ref[key][0], key)
        SR.same_results(key[1], dev[key][1], ref[key][1], key)
    # the session is what it was built to be, counted from the DEVICE leg's results: tests/test_session_ref.py's bounds, those that
    # floats decide halved and at least 1
    ev = SR.events_of_results(dev)
    print("events of the device leg", dict(ev), "needs", dict(world["H"].need), "stored list != fresh count", world["H"].events["stale_nn_list"],
          world["H"].events["stale_cull_list"])
    for k in ev:
        assert ev[k] >= max(SR.CPU_REACHED.get(k, 1) // 2, 1), (k, ev[k])
    for k in ("kept_met_again", "arrival_followed_replaced"):  # (what the results do not show: the model leg's count, equal states given)
        assert world["H"].events[k] >= 1, k


def test_session_invariants(gpu, world):
    """session_ref.check_state - numpy alone, no model - on the device leg's state after every step"""
    for key, (snap, _) in generous(gpu, world).items():
        SR.check_state(snap, key)
    SR.check_state(world["entry"], "entry")


def test_session_tight_capacities_and_guards(gpu, world):
    """NMPcap / OBScap / Wcap / the candidate capacity at exactly the largest need of the session (OBScap: gl_map_fuse's own bound, room
    for every candidate to attach, included): the bytes after every key-frame equal the generous run's, and the 64 guard words behind
    every capacity buffer - and behind the output lists a caller can bring: update_connections' and cull_keyframes' - keep their sentinel
    (leg() checks them in every run).  The lists the wrappers allocate themselves are held to their sentinels by the per-call tests, as
    is one below a capacity."""
    torch, ctx = gpu
    need = world["H"].need
    tight, _ = leg(torch, ctx, world, (need["NMP"], need["NOBS"], need["W"], need["cand"]))
    wide = generous(gpu, world)
    for K in world["sc"]["arrivals"]:
        key = (K, SR.STEPS[-1])
        same_state(tight[key][0], wide[key][0], key)
    for key in wide:
        SR.same_results(key[1], tight[key][1], world["model"][key][1], key)


def test_session_twice_on_one_context(gpu, world):
    """the device leg two times on one context of its own, the second on scratch poisoned with 0xFF (tests/test_gpu_context_state.py):
    the same final bytes, and those of the shared context's run"""
    torch = gpu[0]
    ctx = new_context()
    try:
        def make(torch, ctx):
            return api.GMM(ctx, world["mean"], world["cov"]), bow.Vocabulary.from_arrays(ctx, **world["sc"]["voc"])
        gmm, voc = run(make, torch, ctx)
        ctx._case_gmm = gmm  # (close_context closes it)
        first, _ = leg(torch, ctx, world, generous_caps(world), gmm, voc)
        ctx.set_option("test_scratch_fill", 0xFF)
        second, _ = leg(torch, ctx, world, generous_caps(world), gmm, voc)
        voc.close()
    finally:
        close_context(ctx)
    last = (world["sc"]["arrivals"][-1], SR.STEPS[-1])
    same_state(second[last][0], first[last][0], last)
    same_state(first[last][0], generous(gpu, world)[last][0], last)


@pytest.mark.parametrize("route", ["calls", "host"])
def test_session_split_composites(gpu, world, route):
    """create_map_points_from_map replaced by n_nb = 1 calls of create_map_points_on_map with map_add between them, and
    search_in_neighbors_from_map by its public per-call route - `calls`: fuse_targets / fuse_and_note per target / fuse_candidates / the
    refresh / covis_update one by one on the device; `host`: the split route of tests/test_gpu_covis.py, the graph and the lists in numpy
    from read-backs: the same bytes after every key-frame"""
    torch, ctx = gpu
    split, _ = leg(torch, ctx, world, generous_caps(world), split=route)
    wide = generous(gpu, world)
    for K in world["sc"]["arrivals"]:
        key = (K, SR.STEPS[-1])
        same_state(split[key][0], wide[key][0], key)


def test_session_with_the_mapping_pass_in_one_call(gpu, world):
    """steps 5a .. 6d of every key-frame through ONE api.mapping_pass_from_map call that is given the key-frame tables and the graph:
    the BA, the erase, updateNormalAndDepth of the window's points, the cull, the removal and the graph's own removal - the state after
    every key-frame is the step-by-step run's, so the composite omits nothing the next key-frame reads"""
    torch, ctx = gpu
    one, _ = leg(torch, ctx, world, generous_caps(world), one_pass=True)
    wide = generous(gpu, world)
    for K in world["sc"]["arrivals"]:
        key = (K, SR.STEPS[-1])
        same_state(one[key][0], wide[key][0], key)
        assert one[(K, "5a ba")][1]["culled"] == wide[key][1]["cull_rows"].tolist()
