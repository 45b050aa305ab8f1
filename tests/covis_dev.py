"""The five calls of gmmloc_amd.covis on the device with GUARD words behind every array they may write (tests/test_gpu_covis_cases.py,
tests/test_gpu_covis.py, tests/test_gpu_covis_context.py): the library is called on views of guarded buffers, every output starts as
zeros, and each helper returns host copies after checking the guards.  Test infrastructure."""
import ctypes as C

import numpy as np

from gmmloc_amd import api, covis
from tests.context_pass import run  # (a HIP error ends the session: nothing more is started on a device that has faulted)
from tests.test_gpu_map_stats import Guarded

GRAPH_KEYS = ("cov_kf", "cov_w", "cov_n", "cov_nord", "best_cov")


class DevGraph:
    """a graph (the dict of tests/covis_cases.graph) on the device, guard words behind each of its five arrays"""

    def __init__(self, torch, g):
        self.shape = g["cov_kf"].shape
        self.g = Guarded(torch, **{k: g[k] for k in GRAPH_KEYS})

    @property
    def cov(self):
        return {k: (self.g.t[k].view(self.shape) if k in ("cov_kf", "cov_w") else self.g.t[k]) for k in GRAPH_KEYS}

    def host(self):
        self.g.check()
        return {k: (self.g.host(k).reshape(self.shape) if k in ("cov_kf", "cov_w") else self.g.host(k)).copy() for k in GRAPH_KEYS}


def dev_map(torch, m):
    """the map dict of tests/covis_ref on the device: what covis.covis_update and covis.fuse_candidates take"""
    dt = dict(mp_valid=np.uint8, kf_valid=np.uint8, kf_mp=np.int32, obs_ptr=np.int32, obs_kf=np.int32)
    return {k: torch.from_numpy(np.ascontiguousarray(m[k], dt[k])).cuda() for k in dt}


def _finish(torch, ctx, fn, out):
    def call(torch, ctx):
        ctx.call(lambda _h: fn())
        torch.cuda.synchronize()
    run(call, torch, ctx)
    out.check()
    return {k: out.host(k).copy() for k in out.full}


def d_update(torch, ctx, md, dg, kf, Ccap):
    v, dev = api._map_view(md, False)
    s = covis._cov(dg.cov, dev)[0]
    o = Guarded(torch, conn_kf=np.zeros(Ccap), conn_w=np.zeros(Ccap), n_conn=[0], result=np.zeros(4))
    p = api._ptr
    return _finish(torch, ctx, lambda: ctx.lib.gl_covis_update(ctx.h, C.byref(v), C.byref(s), int(kf), int(Ccap), p(o.t["conn_kf"]), p(o.t["conn_w"]),
                                                               p(o.t["n_conn"]), p(o.t["result"])), o)


def d_remove(torch, ctx, dg, NKF, rows, kf_first, n_cull=None):
    s = covis._cov(dg.cov)[0]
    o = Guarded(torch, rows=np.asarray(rows, np.int32), n=[len(rows) if n_cull is None else n_cull], result=np.zeros(4))
    p = api._ptr
    r = _finish(torch, ctx, lambda: ctx.lib.gl_covis_remove(ctx.h, int(NKF), C.byref(s), int(kf_first), p(o.t["rows"]) if len(rows) else None,
                                                            p(o.t["n"]) if n_cull is not None else None, len(rows), p(o.t["result"])), o)
    assert np.array_equal(r["rows"], np.asarray(rows, np.int32)), "the list was written"
    return r["result"]


def d_best(torch, ctx, dg, NKF, kf_rows, N, Ccap):
    s = covis._cov(dg.cov)[0]
    B = len(kf_rows)
    o = Guarded(torch, kf=np.asarray(kf_rows, np.int32), conn_kf=np.zeros(B * Ccap), conn_w=np.zeros(B * Ccap), n_conn=np.zeros(B), result=np.zeros(4))
    p = api._ptr
    r = _finish(torch, ctx, lambda: ctx.lib.gl_covis_best(ctx.h, int(NKF), C.byref(s), B, p(o.t["kf"]), int(N), int(Ccap), p(o.t["conn_kf"]),
                                                          p(o.t["conn_w"]), p(o.t["n_conn"]), p(o.t["result"])), o)
    return dict(conn_kf=r["conn_kf"].reshape(B, Ccap), conn_w=r["conn_w"].reshape(B, Ccap), n_conn=r["n_conn"], result=r["result"])


def d_targets(torch, ctx, dg, NKF, kf_valid, kf_row, nn, nn2, Tcap):
    s = covis._cov(dg.cov)[0]
    o = Guarded(torch, tgt_kf=np.zeros(Tcap), n_tgt=[0], result=np.zeros(4))
    valid = None if kf_valid is None else torch.from_numpy(np.ascontiguousarray(kf_valid, np.uint8)).cuda()
    p = api._ptr
    return _finish(torch, ctx, lambda: ctx.lib.gl_fuse_targets(ctx.h, int(NKF), C.byref(s), p(valid), int(kf_row), int(nn), int(nn2), int(Tcap),
                                                               p(o.t["tgt_kf"]) if Tcap else None, p(o.t["n_tgt"]), p(o.t["result"])), o)


def d_candidates(torch, ctx, md, tgt, n_tgt, kf_idx, cand_cap):
    v, _ = api._map_view(md, False)
    o = Guarded(torch, tgt=np.asarray(tgt, np.int32), n_tgt=[n_tgt], cand_mp=np.zeros(cand_cap), n_cand=[0], result=np.zeros(4))
    p = api._ptr
    r = _finish(torch, ctx, lambda: ctx.lib.gl_fuse_candidates(ctx.h, C.byref(v), p(o.t["tgt"]) if len(tgt) else None, p(o.t["n_tgt"]), len(tgt),
                                                               int(kf_idx), int(cand_cap), p(o.t["cand_mp"]) if cand_cap else None, p(o.t["n_cand"]),
                                                               p(o.t["result"])), o)
    assert np.array_equal(r["tgt"], np.asarray(tgt, np.int32)) and r["n_tgt"].tolist() == [n_tgt], "the target list was written"
    return {k: r[k] for k in ("cand_mp", "n_cand", "result")}
