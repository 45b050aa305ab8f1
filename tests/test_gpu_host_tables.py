"""The checks the Python host derives from its one table of the resident map's tables (gmmloc_amd/_host.py), through one reader of each
kind - a view reader (api.update_connections), a `ba` reader (api.cull_keyframes), an editor (api.map_remove) and a grower
(map_grow.map_add, the same tensors as capacity buffers with sizes = (2, 1, 3)) - on the smallest map that has every table: NMP = 3,
NKF = 2, NFK = 2, NOBS = 4.  A bad tensor is refused by every reader that is given it, before any C call; _count and Context.call.

obs_ptr, obs_kf and kf_mp ARE the four extents: with a row (or kf_mp a feature slot) too many or too few they are tensors of another
map, and what a reader can refuse is the first table that contradicts them - CONTRADICTS names it.  A reader that is given no such table
has nothing to refuse (update_connections: obs_kf's length, kf_mp's NFK)."""
import ctypes as C

import pytest

from gmmloc_amd import _host, _lib, api, map_grow

pytestmark = pytest.mark.gpu

NMP, NKF, NFK, NOBS = 3, 2, 2, 4
OTHER = {"uint8": "int32", "int32": "int64", "float32": "float64", "float64": "float32"}
CONTRADICTS = {("obs_ptr", "rows"): "map['mp_valid']", ("obs_kf", "rows"): "ba['obs_feat']", ("kf_mp", "rows"): "map['kf_valid']",
               ("kf_mp", "trailing"): "ba['kf_uvr']"}


def the_map(torch):
    """point 0 seen by (kf 0, feat 0) and (kf 1, feat 0), point 1 by (kf 0, feat 1), point 2 by (kf 1, feat 1)"""
    T = lambda a, dt: torch.tensor(a, dtype=getattr(torch, dt), device="cuda")
    m = dict(mp_valid=T([1, 1, 1], "uint8"), obs_ptr=T([0, 2, 3, 4], "int32"), obs_kf=T([0, 1, 0, 1], "int32"), kf_valid=T([1, 1], "uint8"),
             kf_mp=T([[0, 1], [0, 2]], "int32"), mp_pos=T([[0, 0, 4], [1, 0, 4], [0, 1, 5]], "float64"), mp_normal=T([[0, 0, -1]] * 3, "float64"),
             mp_max_dist=T([8, 8, 8], "float32"), mp_min_dist=T([1, 1, 1], "float32"), mp_desc=T([[7] * 32] * 3, "uint8"))
    pose = [0, 0, 0, 0, 0, 0, 1]
    ba = dict(kf_pose=T([pose, pose], "float64"), kf_twc=T([[0, 0, 0], [0.1, 0, 0]], "float64"),
              kf_uvr=T([[[300, 200, 280], [340, 200, -1]], [[290, 200, 270], [300, 240, 285]]], "float64"), kf_oct=T([[0, 1], [0, 0]], "int32"),
              obs_feat=T([0, 0, 1, 1], "int32"), mp_assoc=T([0, -1, 2], "int32"), kf_first=0)
    return m, ba, T([0, 0, 1], "int32")


def readers(torch, ctx, m, ba, rk):
    """name -> (the dicts it is given, the call)"""
    T = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")
    return {"view": (("map",), lambda: api.update_connections(ctx, m, T([1], torch.int32), Ccap=2)),
            "ba": (("map", "ba"), lambda: api.cull_keyframes(ctx, m, ba, T([[3.0, 3.0], [3.0, 3.0]], torch.float32), 6.0, T([[1]], torch.int32),
                                                            T([1], torch.int32))),
            "edit": (("map", "ba", None), lambda: api.map_remove(ctx, m, ba, mp_ref_kf=rk)),
            "grow": (("map", "ba", None), lambda: map_grow.map_add(ctx, m, ba, (2, 1, 3), mp_ref_kf=rk))}


def bad_versions(torch, key, t):
    """(what, kind, the tensor): wrong dtype, a leading row too many, one too few, each trailing extent wrong, not contiguous"""
    yield "dtype", "dtype", t.to(getattr(torch, OTHER[_host.MAP_TABLES[key].dtype]))
    yield "a row too many", "rows", torch.cat([t, t[:1]])
    yield "a row too few", "rows", t[:-1].contiguous()
    for d in range(1, t.dim()):
        yield "trailing extent %d" % d, "trailing", torch.cat([t, t.narrow(d, 0, 1)], d)
    yield "not contiguous", "contiguous", t.repeat_interleave(2, 0)[::2]


class NoLibrary:
    def __getattr__(self, name):
        pytest.fail("the wrapper reached the library (%s) with a bad tensor" % name)


@pytest.mark.parametrize("key", list(_host.MAP_TABLES))
def test_a_bad_table_is_refused_by_every_reader_before_any_c_call(gpu, monkeypatch, key):
    torch, ctx = gpu
    m, ba, rk = the_map(torch)
    where = _host.MAP_TABLES[key].where
    good = {"map": m, "ba": ba, None: {"mp_ref_kf": rk}}[where][key]
    monkeypatch.setattr(ctx, "lib", NoLibrary())
    n = 0
    for what, kind, t in bad_versions(torch, key, good):
        assert not (t.is_contiguous() and t.dtype == good.dtype and t.shape == good.shape), what
        m2, ba2, rk2 = (dict(m, **{key: t}) if where == "map" else m), (dict(ba, **{key: t}) if where == "ba" else ba), (t if where is None else rk)
        named = CONTRADICTS.get((key, kind), "mp_ref_kf" if where is None else "%s[%r]" % (where, key))
        for reader, (given, call) in readers(torch, ctx, m2, ba2, rk2).items():
            if where not in given or (named[:2] == "ba" and "ba" not in given):
                continue
            with pytest.raises(AssertionError) as e:
                call()
            assert str(e.value).startswith(named + ":"), (key, what, reader, str(e.value))
            n += 1
    assert n >= 2 * 4  # (mp_ref_kf: four versions, two readers)


class Recording:
    def __init__(self, lib):
        self.lib, self.views = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(h, *args):
            if isinstance(getattr(args[0], "_obj", None), _lib.gl_map_view):
                v = args[0]._obj
                self.views[name] = (v.NMP, v.NKF, v.NFK, v.NOBS)
            return fn(h, *args)
        return call


def test_the_good_map_is_accepted_by_every_reader(gpu, monkeypatch):
    torch, ctx = gpu
    m, ba, rk = the_map(torch)
    rec = Recording(ctx.lib)
    monkeypatch.setattr(ctx, "lib", rec)
    r = readers(torch, ctx, m, ba, rk)
    conn = r["view"][1]()
    cull = r["ba"][1]()
    rem = r["edit"][1]()
    add = r["grow"][1]()
    torch.cuda.synchronize()
    assert rec.views == {"gl_update_connections": (3, 2, 2, 4), "gl_cull_keyframes": (3, 2, 2, 4)}
    assert conn["n_conn"].tolist() == [1] and conn["conn_kf"][0, 0].item() == 0 and tuple(cull["cull"].shape) == (1, 1)
    assert (rem["nobs"], rem["n_dead"], rem["status"]) == (4, 0, 0) and add["sizes"] == (2, 1, 3) and add["status"] == 0


def test_count_wants_one_int32(gpu):
    torch, _ = gpu
    dev = torch.zeros(1, device="cuda").device
    assert _host._count("n_x", torch.zeros(1, dtype=torch.int32, device=dev), dev).value
    for n in (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)):
        with pytest.raises(AssertionError, match="n_x: one int32 on the device"):
            _host._count("n_x", n, dev)


def test_call_raises_the_library_error_and_closes_the_bracket(gpu):
    torch, ctx = gpu
    m, ba, _ = the_map(torch)
    v, dev = api._map_view(m, False)
    w = api._map_ba_view(ba, v, dev)
    depth = torch.full((NKF, NFK), 3.0, dtype=torch.float32, device=dev)
    with pytest.raises(api.GLError) as e:  # Ccap = 0: refused with GL_ERR_ARG before anything is launched
        ctx.call(ctx.lib.gl_cull_keyframes, C.byref(v), C.byref(w), api._ptr(depth), 6.0, 1, 0, None, None, None, None, None, None, None, None)
    assert str(e.value) == "libgmmloc_hip error -1: " + ctx.lib.gl_last_error_string().decode()
    conn = api.update_connections(ctx, m, torch.tensor([1], dtype=torch.int32, device=dev), Ccap=2)  # (the bracket was closed: the next call runs)
    assert conn["n_conn"].tolist() == [1]
