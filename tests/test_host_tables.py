"""The Python host's one table of the resident map's tables (gmmloc_amd/_host.py: MAP_TABLES) against the structs of the binding table,
map_grow.map_views - which only slices - on plain CPU tensors with the expected extents written out, and _count on what is not on a
device.  No library call."""
import ctypes as C

import pytest
import torch

from gmmloc_amd import _host, _lib, api, map_grow


def fields(struct, pointers):
    """the struct's pointer fields, or its others without the padding word `reserved_` (gl_map_ba_view has one behind kf_first)"""
    return [f for f, t in struct._fields_ if (t is C.c_void_p) == pointers and f != "reserved_"]


def test_every_struct_field_is_a_table_once():
    view, ba = fields(_lib.gl_map_view, True), fields(_lib.gl_map_ba_view, True)
    assert len(set(view + ba)) == len(view + ba)
    assert sorted(k for k, t in _host.MAP_TABLES.items() if t.where == "map") == sorted(view)
    assert sorted(k for k, t in _host.MAP_TABLES.items() if t.where == "ba") == sorted(ba)
    assert sorted(_host.MAP_TABLES) == sorted(view + ba + ["mp_ref_kf"]) and _host.MAP_TABLES["mp_ref_kf"].where is None
    assert fields(_lib.gl_map_view, False) == ["NMP", "NKF", "NFK", "NOBS"] and fields(_lib.gl_map_ba_view, False) == ["kf_first"]
    assert all(t is C.c_void_p and f in _host.MAP_TABLES for f, t in _lib.gl_map_edit._fields_)
    # what the other modules import is the table's, in the structs' order
    assert list(api.MAP_VIEW_DTYPES) == view and list(api.MAP_BA_DTYPES) == ba
    assert {k: _host.MAP_TABLES[k].dtype for k in view + ba} == dict(api.MAP_VIEW_DTYPES, **api.MAP_BA_DTYPES)
    assert api.MAP_VIEW_POINT_KEYS == ("mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc")


def test_map_views_cuts_each_table_by_its_extent():
    NMPcap, KF, NFK, OBScap = 5, 3, 2, 7
    z = lambda *sh: torch.zeros(sh)
    m = dict(mp_valid=z(NMPcap), obs_ptr=z(NMPcap + 1), obs_kf=z(OBScap), kf_valid=z(KF), kf_mp=z(KF, NFK), mp_pos=z(NMPcap, 3), mp_normal=z(NMPcap, 3),
             mp_max_dist=z(NMPcap), mp_min_dist=z(NMPcap), mp_desc=z(NMPcap, 32))
    ba = dict(kf_pose=z(KF, 7), kf_twc=None, kf_uvr=z(KF, NFK, 3), kf_oct=z(KF, NFK), obs_feat=z(OBScap), mp_assoc=z(NMPcap), kf_first=1)
    m2, b2 = map_grow.map_views(m, ba, (3, 2, 4))
    want_m = dict(mp_valid=(3,), obs_ptr=(4,), obs_kf=(4,), kf_valid=(2,), kf_mp=(2, 2), mp_pos=(3, 3), mp_normal=(3, 3), mp_max_dist=(3,), mp_min_dist=(3,),
                  mp_desc=(3, 32))
    want_b = dict(kf_pose=(2, 7), kf_uvr=(2, 2, 3), kf_oct=(2, 2), obs_feat=(4,), mp_assoc=(3,))
    assert set(m2) == set(m) and set(b2) == set(ba)
    for got, src, want in ((m2, m, want_m), (b2, ba, want_b)):
        for k, sh in want.items():
            assert tuple(got[k].shape) == sh, (k, tuple(got[k].shape))
            assert got[k].data_ptr() == src[k].data_ptr(), k
    assert b2["kf_first"] == 1 and isinstance(b2["kf_first"], int) and b2["kf_twc"] is None


def test_count_wants_a_device_tensor():
    assert _host._count("n_x", None, torch.device("cpu")) is None
    with pytest.raises(AssertionError, match="n_x: one int32 on the device"):
        _host._count("n_x", torch.zeros(1, dtype=torch.int32), torch.device("cpu"))
