"""The Python host's plumbing, stated once for every wrapper module: the error check, the argument checks, the resident map's tables
with the structs built from them, and the `out` dict of a call that may be given its outputs.  Imports only _lib; api.py re-exports
what tests and tools reach for."""
import ctypes as C
from collections import namedtuple

from . import _lib


class GLError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise GLError("libgmmloc_hip error %d: %s" % (rc, _lib.load().gl_last_error_string().decode()))


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device buffers must be contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


def _tensor(name, t, dtype, shape, device):
    """`t` is a contiguous CUDA tensor of that dtype and shape (None in the shape: any extent) on `device` - or raise."""
    assert t is not None, "%s: missing" % name
    assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dtype, \
        "%s: expected a contiguous CUDA %s tensor, got %s%s" % (name, dtype, t.dtype, "" if t.is_contiguous() else " (not contiguous)")
    assert device is None or t.device == device, "%s: on %s, expected %s" % (name, t.device, device)
    assert t.dim() == len(shape) and all(w is None or int(w) == int(h) for w, h in zip(shape, t.shape)), \
        "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
    return t


def _count(name, n, dev):
    """a device-side length: None, or one int32 on the device -> its pointer"""
    if n is None:
        return None
    assert n.is_cuda and n.device == dev and str(n.dtype) == "torch.int32" and n.numel() == 1, "%s: one int32 on the device" % name
    return _ptr(n)


def _outputs(out, spec, dev):
    """`out`: the dict of an earlier call, used again, or None: a fresh one.  spec: name -> (dtype, shape, fill); every tensor of it is
    checked either way."""
    import torch
    if out is None:
        out = {k: torch.full(sh, fill, dtype=getattr(torch, dt), device=dev) for k, (dt, sh, fill) in spec.items()}
    for k, (dt, sh, _) in spec.items():
        _tensor("out[%r]" % k, out.get(k), dt, sh, dev)
    return out


# ---- the resident map's tables: dtype, the extent the leading dimension follows, the trailing shape, the dict that holds it (`map`: the
# arrays of gl_map_view, `ba`: those of gl_map_ba_view; mp_ref_kf travels on its own).  Every check of a map below reads this and nothing else.
Table = namedtuple("Table", "dtype lead trail where")
MAP_TABLES = {
    "mp_valid": Table("uint8", "NMP", (), "map"), "obs_ptr": Table("int32", "NMP + 1", (), "map"), "obs_kf": Table("int32", "NOBS", (), "map"),
    "kf_valid": Table("uint8", "NKF", (), "map"), "kf_mp": Table("int32", "NKF", ("NFK",), "map"), "mp_pos": Table("float64", "NMP", (3,), "map"),
    "mp_normal": Table("float64", "NMP", (3,), "map"), "mp_max_dist": Table("float32", "NMP", (), "map"),
    "mp_min_dist": Table("float32", "NMP", (), "map"), "mp_desc": Table("uint8", "NMP", (32,), "map"),
    "kf_pose": Table("float64", "NKF", (7,), "ba"), "kf_twc": Table("float64", "NKF", (3,), "ba"), "kf_uvr": Table("float64", "NKF", ("NFK", 3), "ba"),
    "kf_oct": Table("int32", "NKF", ("NFK",), "ba"), "obs_feat": Table("int32", "NOBS", (), "ba"), "mp_assoc": Table("int32", "NMP", (), "ba"),
    "mp_ref_kf": Table("int32", "NMP", (), None)}
# The whole map as device arrays (gl_map_view): what update_map_points reads and writes + the key-frames' mappoints_ table.
MAP_VIEW_DTYPES = {k: t.dtype for k, t in MAP_TABLES.items() if t.where == "map"}
MAP_BA_DTYPES = {k: t.dtype for k, t in MAP_TABLES.items() if t.where == "ba"}
MAP_VIEW_POINT_KEYS = tuple(k for k in MAP_VIEW_DTYPES if MAP_TABLES[k].lead == "NMP" and k != "mp_valid")
_SIZED_BY = ("obs_ptr", "obs_kf", "kf_mp")  # the three tables every map holds: their shapes ARE the four extents
_VIEW_REST = tuple(k for k in MAP_VIEW_DTYPES if k not in _SIZED_BY)
_CHECK = {k: ("%s[%r]" % (t.where, k) if t.where else k, t.dtype, (t.lead,) + t.trail) for k, t in MAP_TABLES.items()}  # (the name in a message)


def _extents(NMP, NKF, NFK, NOBS):
    return {"NMP": NMP, "NMP + 1": None if NMP is None else NMP + 1, "NKF": NKF, "NFK": NFK, "NOBS": NOBS}


_ANY = _extents(None, None, None, None)


def _table(d, k, ext, dev):
    """d[k] is table k for the extents `ext` (of _extents; _ANY: whatever it has) - or raise, naming the dict and the key"""
    name, dtype, dims = _CHECK[k]
    return _tensor(name, d.get(k), dtype, tuple(map(ext.get, dims, dims)), dev)  # (a number in dims stands for itself)


def _map_extents(m):
    """the keys of `map` and its three sizing tables -> (rows of the per-point arrays, key-frame rows, NFK, observation entries, device)"""
    for k in m:
        assert k in MAP_VIEW_DTYPES, "map[%r]: unknown key" % k
    dev = _table(m, "obs_ptr", _ANY, None).device
    NMP = m["obs_ptr"].shape[0] - 1
    assert NMP >= 0, "map['obs_ptr']: needs NMP + 1 entries"
    NOBS = _table(m, "obs_kf", _ANY, dev).shape[0]
    NKF, NFK = _table(m, "kf_mp", _ANY, dev).shape
    return NMP, NKF, NFK, NOBS, dev


def _map_view(m, need_points):
    """dict of CUDA tensors -> (gl_map_view, device).  Keys of MAP_VIEW_DTYPES; mp_valid / kf_valid optional (all valid); the per-point
    arrays only where `need_points`."""
    NMP, NKF, NFK, NOBS, dev = _map_extents(m)
    ext = _extents(NMP, NKF, NFK, NOBS)
    v = _lib.gl_map_view()
    v.NMP, v.NKF, v.NFK, v.NOBS = NMP, NKF, NFK, NOBS
    for k in _SIZED_BY:
        setattr(v, k, m[k].data_ptr())
    for k in _VIEW_REST:
        if m.get(k) is not None or (need_points and k in MAP_VIEW_POINT_KEYS):
            setattr(v, k, _table(m, k, ext, dev).data_ptr())
    return v, dev


def _map_ba_view(ba, v, dev, need=None):
    """dict of CUDA tensors (keys of MAP_BA_DTYPES; kf_twc optional; `need`: the keys a call reads when it does not read them all) +
    kf_first (int, -1: none) -> gl_map_ba_view for the map view v"""
    for k in ba:
        assert k in MAP_BA_DTYPES or k == "kf_first", "ba[%r]: unknown key" % k
    ext = _extents(v.NMP, v.NKF, v.NFK, v.NOBS)
    w = _lib.gl_map_ba_view()
    for k in MAP_BA_DTYPES:
        if ba.get(k) is None and (k == "kf_twc" or (need is not None and k not in need)):
            continue
        setattr(w, k, _table(ba, k, ext, dev).data_ptr())
    w.kf_first = int(ba.get("kf_first", -1))
    return w


def _map_buffers(map, ba, sizes, need_ba):
    """the two dicts as CAPACITY buffers (map_grow's module docstring): every tensor they hold checked against the capacities, `sizes`
    inside them -> (NMP, NKF, NFK, NOBS, NMPcap, OBScap, device)"""
    NMPcap, KFcap, NFK, OBScap, dev = _map_extents(map)
    for k in ba:
        assert k in MAP_BA_DTYPES or k == "kf_first", "ba[%r]: unknown key" % k
    NMP, NKF, NOBS = (NMPcap, KFcap, OBScap) if sizes is None else (int(v) for v in sizes)
    assert 0 <= NMP <= NMPcap and 0 <= NKF <= KFcap and 0 <= NOBS <= OBScap, \
        "sizes %s outside the buffers (NMPcap %d, key-frame rows %d, OBScap %d)" % ((NMP, NKF, NOBS), NMPcap, KFcap, OBScap)
    assert map.get("mp_valid") is not None and map.get("kf_valid") is not None, "mp_valid and kf_valid are written, both are needed"
    ext = _extents(NMPcap, KFcap, NFK, OBScap)
    for d, keys in ((map, _VIEW_REST), (ba, MAP_BA_DTYPES)):
        for k in keys:
            if d.get(k) is not None or k == "obs_feat":
                _table(d, k, ext, dev)
    for k in need_ba:
        assert ba.get(k) is not None, "ba[%r]: missing" % k
    return NMP, NKF, NFK, NOBS, NMPcap, OBScap, dev


def _map_edit(map, ba, mp_ref_kf, rows, dev):
    """gl_map_edit from the two dicts, their tensors already checked, and mp_ref_kf (rows,) i32 or None.  A table that is not there
    stays NULL: which ones a call needs is the caller's statement."""
    src = {"map": map, "ba": ba, None: {"mp_ref_kf": mp_ref_kf}}
    if mp_ref_kf is not None:
        _table(src[None], "mp_ref_kf", {"NMP": rows}, dev)
    ed = _lib.gl_map_edit()
    for k, _ in ed._fields_:
        setattr(ed, k, _ptr(src[MAP_TABLES[k].where].get(k)))
    return ed
