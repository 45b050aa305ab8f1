#!/usr/bin/env python3
"""Times of what ADDS to the resident map, one JSON line per run:
    python tools/map_grow_time.py kernels [reps]  (a) device time (HIP events around ONE call each, the map restored before it) of
                                                  gl_map_add - a new key-frame walked, 12 new points with two triples each, 40 colliding
                                                  triples - and of gl_map_fuse - 120 candidates onto six slots of one key-frame - on the
                                                  `small` and `euroc` scenes of tests/map_grow_scenes.py; `small` checked against
                                                  tests/map_grow_ref.py first
    python tools/map_grow_time.py device [reps]   (b) host to host on `euroc`: one key-frame's additions - map_add, then map_fuse - on the
                                                  resident map: two read-backs of 24 and 20 bytes, nothing uploaded but the lists
    python tools/map_grow_time.py upload [reps]   (c) the route without the two calls, a host that does NO flattening: the CSR and the
                                                  kf_mp / validity rows ALREADY EDITED in page-locked memory are uploaded after the
                                                  additions and again after the fuse (the host's own edit is not priced).  A lower bound
                                                  of the host path.
    python tools/map_grow_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated
                                                  three times, stopping at the first failure; the lines are also written to out.txt
Host to host: wall clock around one pass that ends in a synchronise, median / min / max; the map is restored before every timed pass
(outside the timed part)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
STEP_LIMIT_S = 240


def run_all():
    out = sys.argv[3] if len(sys.argv) > 3 else None
    lines = []
    for leg in ["kernels"] + ["device", "upload"] * 3:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), leg, str(REPS)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("leg %s failed (exit status %d): stopping" % (leg, r.returncode))
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if MODE == "all":
    run_all()
    raise SystemExit(0)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import _lib, api, map_grow  # noqa: E402
from tests import map_edit_scenes as ES  # noqa: E402
from tests import map_grow_ref as G  # noqa: E402
from tests import map_grow_scenes as GS  # noqa: E402

ctx = gmmloc_amd.Context(0)
MUTABLE = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")


def T(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def padded(a, n):
    out = np.zeros((n,) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


class Resident:
    """a scene whose key-frame is NEW again, in capacity buffers on the device, the lists of one mapping pass, and a copy of what the two
    calls change"""

    def __init__(self, name):
        self.m, self.ba, self.ref, self.ls = GS.add_lists(ES.scene(name, name in ES.CLAMP), 2)
        m, ba, ls = self.m, self.ba, self.ls
        self.rows1, self.res1 = G.map_add(m, ba, self.ref, ls["new_mp"], ls["new_kf"], ls["attach"], ls["walk_kf"]) if name == "small" else (None, None)
        NMP, NOBS = len(m["mp_valid"]), len(m["obs_kf"])
        self.sizes = (NMP, len(m["kf_valid"]), NOBS)
        n_req = len(ls["attach"]) + len(ls["walk_kf"]) * m["kf_mp"].shape[1]
        self.caps = (NMP + len(ls["new_mp"]["pos"]), NOBS + n_req + 200)
        per_point = lambda a: padded(np.asarray(a), self.caps[0])
        per_obs = lambda a: padded(np.asarray(a), self.caps[1])
        self.md = dict(mp_valid=T(per_point(m["mp_valid"]), np.uint8), kf_valid=T(m["kf_valid"], np.uint8), kf_mp=T(m["kf_mp"]), obs_kf=T(per_obs(m["obs_kf"])),
                       obs_ptr=T(padded(m["obs_ptr"], self.caps[0] + 1)), mp_pos=T(per_point(m["mp_pos"]), np.float64))
        self.bd = dict(kf_uvr=T(ba["kf_uvr"], np.float64), obs_feat=T(per_obs(ba["obs_feat"])), mp_assoc=T(per_point(ba["mp_assoc"])), kf_first=ba["kf_first"])
        self.rk = T(per_point(self.ref))
        self.keep = {k: self.md[k].clone() for k in MUTABLE}
        self.keep_feat, self.keep_ref = self.bd["obs_feat"].clone(), self.rk.clone()
        a = ls["attach"]
        self.add_kw = dict(new_mp=dict(pos=T(ls["new_mp"]["pos"], np.float64), assoc=T(ls["new_mp"]["assoc"]), ref_kf=T(ls["new_mp"]["ref_kf"])),
                           new_kf=T(ls["new_kf"]), attach=dict(mp=T(a[:, 0]), kf=T(a[:, 1]), feat=T(a[:, 2])), walk_kf=T(ls["walk_kf"]))

    def restore(self):
        for k, v in self.keep.items():
            self.md[k].copy_(v)
        self.bd["obs_feat"].copy_(self.keep_feat)
        self.rk.copy_(self.keep_ref)

    def keep_now(self):
        """what restore() brings back from now on: the map as it stands"""
        self.keep = {k: self.md[k].clone() for k in MUTABLE}
        self.keep_feat, self.keep_ref = self.bd["obs_feat"].clone(), self.rk.clone()


def event_us(fn, restore, n):
    """device time of ONE call between two events, n times"""
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 3):
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            fn()
            e1.record(ctx.stream)
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(1e3 * e0.elapsed_time(e1))
    return stats(ts)


def wall_us(fn, restore, n):
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 5):
            restore()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 5:
                ts.append(1e6 * (time.perf_counter() - t))
    return stats(ts)


def fuse_lists_on_grown(rs):
    """the fuse list of the key-frame that holds the most points, on the map as the add leaves it (read back once, outside any timing)"""
    a = map_grow.map_add(ctx, rs.md, rs.bd, rs.sizes, mp_ref_kf=rs.rk, **rs.add_kw)
    torch.cuda.synchronize()
    assert a["status"] == 0
    m1 = {k: a["map"][k].cpu().numpy() for k in MUTABLE}
    kf, cand, best = GS.fuse_lists(dict(m=m1), 1)
    return a, m1, kf, cand, best


def kernels_leg():
    res = {"mode": "kernels", "device": torch.cuda.get_device_name(0), "reps": REPS}
    p, ref_ = api._ptr, C.byref
    for name in ("small", "euroc"):
        rs = Resident(name)
        NMP, NKF, NOBS = rs.sizes
        NFK = rs.m["kf_mp"].shape[1]
        a, m1, kf, cand, best = fuse_lists_on_grown(rs)
        same = None
        if name == "small":
            same = a["sizes"] == (rs.res1[0], NKF, rs.res1[1]) and all(m1[k].tobytes() == rs.rows1[k].tobytes() for k in MUTABLE) \
                and a["ba"]["obs_feat"].cpu().numpy().tobytes() == rs.rows1["obs_feat"].tobytes()
            assert same, name
        # the library calls themselves on structs made once (the wrappers' validation costs more host time than the kernels run)
        ed = api._map_edit(rs.md, rs.bd, rs.rk, rs.caps[0], rs.rk.device)
        kw = rs.add_kw
        ls = _lib.gl_map_add_lists()
        ls.new_pos, ls.new_assoc, ls.new_ref_kf, ls.new_mp_cap = p(kw["new_mp"]["pos"]), p(kw["new_mp"]["assoc"]), p(kw["new_mp"]["ref_kf"]), len(kw["new_mp"]["assoc"])
        ls.new_kf, ls.new_kf_cap = p(kw["new_kf"]), len(kw["new_kf"])
        ls.att_mp, ls.att_kf, ls.att_feat, ls.attach_cap = p(kw["attach"]["mp"]), p(kw["attach"]["kf"]), p(kw["attach"]["feat"]), len(kw["attach"]["mp"])
        ls.walk_kf, ls.walk_cap = p(kw["walk_kf"]), len(kw["walk_kf"])
        result, already = torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(ls.walk_cap * NFK, dtype=torch.int32, device="cuda")
        o = _lib.gl_map_add_out()
        o.result, o.already_mp, o.already_cap = p(result), p(already), ls.walk_cap * NFK
        ta = event_us(lambda: ctx.lib.gl_map_add(ctx.h, NMP, NKF, NFK, NOBS, rs.caps[0], rs.caps[1], ref_(ed), p(rs.md["mp_pos"]), p(rs.bd["mp_assoc"]), ref_(ls), ref_(o)),
                      rs.restore, REPS)
        after_add = result.tolist()
        rs.keep_now()  # the fuse is timed on the grown map
        cand_d, best_d = T(cand), T(best)
        fres, src, tgt = torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(len(cand), dtype=torch.int32, device="cuda"), torch.zeros(len(cand), dtype=torch.int32, device="cuda")
        fo = _lib.gl_map_fuse_out()
        fo.result, fo.repl_src, fo.repl_tgt, fo.repl_cap = p(fres), p(src), p(tgt), len(cand)
        tf = event_us(lambda: ctx.lib.gl_map_fuse(ctx.h, after_add[0], NKF, NFK, after_add[1], rs.caps[1], ref_(ed), p(rs.bd["kf_uvr"]), kf, len(cand), p(cand_d), p(best_d),
                                                  ref_(fo)), rs.restore, REPS)
        res[name] = {"NMP": NMP, "NKF": NKF, "NFK": NFK, "NOBS": NOBS, "add_lists": [ls.new_mp_cap, ls.new_kf_cap, ls.attach_cap, ls.walk_cap],
                     "add_result": after_add, "add_device_us_median_min_max": ta, "fuse_candidates": len(cand), "fuse_result": fres.tolist(),
                     "fuse_device_us_median_min_max": tf, "add_equal_to_model": same}
    print(json.dumps(res))


def pass_legs():
    rs = Resident("euroc")
    NMP, NKF, NOBS = rs.sizes
    res = {"mode": MODE, "reps": REPS, "NMP": NMP, "NKF": NKF, "NFK": int(rs.m["kf_mp"].shape[1]), "NOBS": NOBS}
    a, m1, kf, cand, best = fuse_lists_on_grown(rs)
    rs.restore()
    if MODE == "device":
        cand_d, best_d = T(cand), T(best)
        out = {}

        def call():
            out["a"] = map_grow.map_add(ctx, rs.md, rs.bd, rs.sizes, mp_ref_kf=rs.rk, **rs.add_kw)
            out["f"] = map_grow.map_fuse(ctx, rs.md, rs.bd, kf, cand_d, best_d, sizes=out["a"]["sizes"])
        res["host_to_host_us_median_min_max"] = wall_us(call, rs.restore, REPS)
        n_list = 5 * len(rs.ls["new_mp"]["pos"]) + len(rs.ls["new_kf"]) + 3 * len(rs.ls["attach"]) + len(rs.ls["walk_kf"]) + 2 * len(cand)
        res.update(attached=out["a"]["n_attached"], fused=out["f"]["n_fused"], replaced=out["f"]["n_replaced"], nobs_after=out["f"]["sizes"][2],
                   bytes_up=4 * n_list + 16 * len(rs.ls["new_mp"]["pos"]), bytes_down=44)
    elif MODE == "upload":
        keys = MUTABLE + ("obs_feat",)
        tgt = {k: (rs.md[k] if k in rs.md else rs.bd[k]) for k in keys}
        host = {k: tgt[k].cpu().pin_memory() for k in keys}  # (the sizes are what counts: the host's edit is not priced)

        def call():
            for k in keys:  # the host's rows after its own additions
                tgt[k].copy_(host[k], non_blocking=True)
            for k in keys:  # ... and after its own fuse
                tgt[k].copy_(host[k], non_blocking=True)
        res["host_to_host_us_median_min_max"] = wall_us(call, lambda: None, REPS)
        res.update(bytes_up=int(2 * sum(v.numel() * v.element_size() for v in host.values())), bytes_down=0)
    else:
        raise SystemExit("mode: kernels | device | upload | all")
    print(json.dumps(res))


if __name__ == "__main__":
    if MODE == "kernels":
        kernels_leg()
    else:
        pass_legs()
