"""The DBoW2 vocabulary on the device and ORBVocabulary::transform (orb_vocabulary.cpp:20-40): gl_voc_*, gl_bow_transform; the
rules and the declared behaviours are in include/gmmloc_hip.h.

A vocabulary is the four record arrays of its nodes 1 .. n (the root, node 0, has no record): parent (n,) i32, desc (n,32) u8, weight
(n,) f32, is_leaf (n,) u8, with k and L of the file's header.  `transform` only enqueues: what it returns are device tensors."""
import ctypes as C

import numpy as np

from . import _lib
from ._host import _check, _ptr, _tensor

BOW_NODES_TRUNCATED = 1
BOW_MAX_FEATURES = 4096
FV_KEYS = ("nnode", "node_id", "node_ptr", "node_idx")


def read_vocabulary_file(path):
    """gl_voc_file_read (host only) -> dict(parent, desc, weight, is_leaf, k, L)"""
    lib = _lib.load()
    n, kl = C.c_int(0), (C.c_int * 2)()
    _check(lib.gl_voc_file_read(str(path).encode(), None, None, None, None, 0, C.byref(n), kl))
    n_rec = n.value - 1
    v = dict(parent=np.zeros(n_rec, np.int32), desc=np.zeros((n_rec, 32), np.uint8), weight=np.zeros(n_rec, np.float32),
             is_leaf=np.zeros(n_rec, np.uint8))
    _check(lib.gl_voc_file_read(str(path).encode(), v["parent"].ctypes.data, v["desc"].ctypes.data, v["weight"].ctypes.data,
                                v["is_leaf"].ctypes.data, n_rec, C.byref(n), kl))
    v.update(k=kl[0], L=kl[1])
    return v


class Vocabulary:
    """gl_voc_t: ORBVocabulary (TemplatedVocabulary<FORB::TDescriptor, FORB>) on the device; immutable."""

    def __init__(self):
        raise TypeError("use Vocabulary.from_file / Vocabulary.from_arrays")

    @classmethod
    def _wrap(cls, ctx, h):
        self = cls.__new__(cls)
        self.ctx, self.lib, self.h = ctx, ctx.lib, h
        return self

    @classmethod
    def from_file(cls, ctx, path):
        """ORBVocabulary::loadFromBinaryFile (TemplatedVocabulary.h:1477-1522)"""
        h = C.c_void_p()
        _check(ctx.lib.gl_voc_load_file(ctx.h, str(path).encode(), C.byref(h)))
        return cls._wrap(ctx, h)

    @classmethod
    def from_arrays(cls, ctx, parent, desc, weight, is_leaf, k, L):
        parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        n = parent.shape[0]
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(n, 32)
        weight = np.ascontiguousarray(weight, dtype=np.float32).reshape(n)
        is_leaf = np.ascontiguousarray(is_leaf, dtype=np.uint8).reshape(n)
        h = C.c_void_p()
        _check(ctx.lib.gl_voc_create(ctx.h, n + 1, parent.ctypes.data, desc.ctypes.data, weight.ctypes.data, is_leaf.ctypes.data, int(k), int(L),
                                     C.byref(h)))
        return cls._wrap(ctx, h)

    def info(self):
        v = (C.c_double * 7)()
        _check(self.lib.gl_voc_info(self.h, v))
        return dict(nodes=int(v[0]), words=int(v[1]), k=int(v[2]), L=int(v[3]), max_children=int(v[4]), min_leaf_level=int(v[5]),
                    device_bytes=int(v[6]))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gl_voc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def feature_vector_alloc(B, NF, nn_cap, device="cuda", fill=0):
    """the CSR arrays of B frames: nnode (B,), node_id (B,nn_cap), node_ptr (B,nn_cap+1), node_idx (B,NF), all int32"""
    import torch
    z = lambda *sh: torch.full(sh, fill, dtype=torch.int32, device=device)
    return dict(nnode=z(B), node_id=z(B, nn_cap), node_ptr=z(B, nn_cap + 1), node_idx=z(B, NF))


def transform(ctx, voc, desc, oct=None, levelsup=4, nn_cap=None, out=None, per_feature=True):
    """gl_bow_transform: desc (B,NF,32) u8, oct (B,NF) i32 or None (< 0: padding slot) -> dict of device tensors: the feature vector as CSR
    (FV_KEYS, as search_by_bow / search_for_triangulation / the chain read it), status (B,) i32 (BOW_NODES_TRUNCATED) and, with
    per_feature, word_id / node (B,NF) i32 and weight (B,NF) f32.  nn_cap defaults to the slots of out['node_id'], else NF (given both, they must agree); `out` supplies any of the arrays (they are
    written in place; the CSR arrays of a truncated frame and the entries behind a frame's counts stay as they are)."""
    import torch
    dev = _tensor("desc", desc, "uint8", (None, None, 32), None).device
    B, NF = desc.shape[:2]
    if oct is not None:
        _tensor("oct", oct, "int32", (B, NF), dev)
    out = dict(out) if out else {}
    if out.get("node_id") is not None:
        assert nn_cap is None or int(nn_cap) == out["node_id"].shape[1], "nn_cap %s, out['node_id'] has %d node slots" % (nn_cap, out["node_id"].shape[1])
        nn_cap = out["node_id"].shape[1]
    nn_cap = NF if nn_cap is None else int(nn_cap)
    shapes = {"word_id": (B, NF), "node": (B, NF), "weight": (B, NF), "nnode": (B,), "node_id": (B, nn_cap), "node_ptr": (B, nn_cap + 1),
              "node_idx": (B, NF), "status": (B,)}
    for key, sh in shapes.items():  # only what the caller did not bring
        if out.get(key) is None and (per_feature or key not in ("word_id", "node", "weight")):
            out[key] = torch.zeros(sh, dtype=torch.float32 if key == "weight" else torch.int32, device=dev)
    o = _lib.gl_bow_out()
    for key, sh in shapes.items():
        if out.get(key) is not None:
            setattr(o, key, _ptr(_tensor("out[%r]" % key, out[key], "float32" if key == "weight" else "int32", sh, dev)))
    ctx.call(ctx.lib.gl_bow_transform, voc.h, int(levelsup), B, NF, nn_cap, _ptr(desc), _ptr(oct), C.byref(o))
    return out


def transform_into_tables(ctx, voc, tables, row, oct=None, levelsup=4):
    """One key-frame's feature vector written in place into row `row` of the gl_map_kf_tables arrays (map_grow.KF_TABLE_DTYPES:
    tables['desc'][row] is read; nnode / node_id / node_ptr / node_idx [row] are written through row views).  oct: (NFK,) i32 or None.
    -> status (1,) i32 on the device."""
    row = int(row)
    assert 0 <= row < tables["desc"].shape[0], "row %d outside the tables" % row
    view = {key: tables[key][row:row + 1] for key in FV_KEYS}
    r = transform(ctx, voc, tables["desc"][row:row + 1], None if oct is None else oct.reshape(1, -1), levelsup=levelsup, out=view, per_feature=False)
    return r["status"]
