#!/usr/bin/env python3
"""Times of the edits of the resident map, one JSON line per run:
    python tools/map_edit_time.py kernels [reps]  (a) device time (HIP events around ONE call each, the map restored before it) of
                                                  gl_cull_keyframes - one list, the first 40 valid key-frames - and of gl_map_remove -
                                                  points, observations and key-frames together - on the `small` and `euroc` scenes of
                                                  tests/map_edit_scenes.py (octaves clamped to <= 1 so that key-frames are culled); `small`
                                                  checked against tests/map_edit_ref.py first, `euroc`'s verdicts against its second form
    python tools/map_edit_time.py device [reps]   (b) host to host on `euroc`: what follows a key-frame's local BA - map_remove(erase_obs)
                                                  -> update_connections -> cull_keyframes -> map_remove(cull_rows) - on the resident map:
                                                  two 12-byte read-backs, nothing uploaded but the erase list
    python tools/map_edit_time.py upload [reps]   (c) the route without gl_map_remove, a host that does NO flattening: the CSR and kf_mp /
                                                  validity rows ALREADY EDITED in page-locked memory are uploaded after the erase, then
                                                  update_connections, then (the culling itself runs on the host and is not priced) uploaded
                                                  again after the cull.  A lower bound of the host path.  Uses entry points the parent
                                                  commit has, so GMMLOC_HIP_LIB may name a build of it.
    python tools/map_edit_time.py all [reps] [out.txt]   every leg in a process of its own with a time limit, (b) and (c) alternated
                                                  three times, stopping at the first failure; the lines are also written to out.txt
The local BA itself is the same call on either route and is left out of (b) and (c).  Host to host: wall clock around one pass that
ends in a synchronise, median / min / max; the map is restored before every timed pass (outside the timed part)."""
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

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import api  # noqa: E402
from tests import ba_window_ref as R  # noqa: E402
from tests import map_edit_scenes as ES  # noqa: E402

ctx = gmmloc_amd.Context(0)
MUTABLE = ("mp_valid", "kf_valid", "kf_mp", "obs_ptr", "obs_kf")


def dev(d):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items() if v is not None}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stats(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def scene(name):
    sc = ES.scene(name)
    sc["ba"]["kf_oct"] = np.minimum(sc["ba"]["kf_oct"], 1).astype(np.int32)
    return sc


class Resident:
    """the scene on the device + a copy of what an edit changes"""

    def __init__(self, sc):
        self.md, self.bd = dev(sc["m"]), dev(sc["ba"])
        self.ref_kf = T(sc["mp_ref_kf"].copy())
        self.keep = {k: self.md[k].clone() for k in MUTABLE}
        self.keep_feat, self.keep_ref = self.bd["obs_feat"].clone(), self.ref_kf.clone()

    def restore(self):
        for k, v in self.keep.items():
            self.md[k].copy_(v)
        self.bd["obs_feat"].copy_(self.keep_feat)
        self.ref_kf.copy_(self.keep_ref)


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


def kernels_leg():
    import ctypes as C
    from gmmloc_amd import _lib
    from tests import map_edit_ref as E
    res = {"mode": "kernels", "device": torch.cuda.get_device_name(0), "reps": REPS}
    for name in ("small", "euroc"):
        sc = scene(name)
        m, ba = sc["m"], sc["ba"]
        NMP, NKF, NFK, NOBS = R._sizes(m)
        rm_mp, erase, rm_kf = ES.removals(sc, 3, n_mp=NMP // 200, n_kf=8, erase_frac=0.002)
        rs = Resident(sc)
        depth, cand, n_cand = T(sc["kf_depth"]), T(sc["cand"][None]), torch.tensor([len(sc["cand"])], dtype=torch.int32, device="cuda")
        out = api.cull_keyframes(ctx, rs.md, rs.bd, depth, sc["th_depth"], cand, n_cand)
        torch.cuda.synchronize()
        ref = E.cull_by_state(m, ba, sc["cand"], sc["kf_depth"], sc["th_depth"])
        n_cull = int(out["n_cull"][0])
        same = np.array_equal(out["cull"][0].cpu().numpy(), ref["cull"]) and np.array_equal(out["num_redundant"][0].cpu().numpy(), ref["num_redundant"]) \
            and np.array_equal(out["cull_rows"][0, :n_cull].cpu().numpy(), ref["cull_rows"])
        if name == "small":
            rows, _ = E.map_remove(m, ba, rm_mp, erase, rm_kf, sc["mp_ref_kf"])
            r = api.map_remove(ctx, rs.md, rs.bd, erase_obs=T(erase), rm_kf=T(rm_kf), rm_mp=T(rm_mp), mp_ref_kf=rs.ref_kf)
            same = same and r["nobs"] == len(rows["obs_kf"]) and all(rs.md[k].cpu().numpy().tobytes() == rows[k].tobytes() for k in ("mp_valid", "kf_valid", "kf_mp", "obs_ptr")) \
                and r["map"]["obs_kf"].cpu().numpy().tobytes() == rows["obs_kf"].tobytes() and np.array_equal(r["dead_mp"].cpu().numpy(), rows["dead_mp"])
        assert same, name
        # the library calls themselves on structs made once (the wrappers' validation costs more host time than the kernels run)
        v, dv = api._map_view(rs.md, False)
        bv = api._map_ba_view(rs.bd, v, dv)
        p, ref_ = api._ptr, C.byref
        rs.restore()
        tc = event_us(lambda: ctx.lib.gl_cull_keyframes(ctx.h, ref_(v), ref_(bv), p(depth), float(sc["th_depth"]), 1, cand.shape[1], p(cand), p(n_cand), p(out["cull"]),
                                                        p(out["num_mps"]), p(out["num_redundant"]), p(out["cand_status"]), p(out["cull_rows"]), p(out["n_cull"])),
                      lambda: None, REPS)
        ed = _lib.gl_map_edit()
        for k in MUTABLE:
            setattr(ed, k, p(rs.md[k]))
        ed.obs_feat, ed.mp_ref_kf = p(rs.bd["obs_feat"]), p(rs.ref_kf)
        lists = [T(rm_mp), T(erase), T(rm_kf)]
        ls = _lib.gl_map_remove_lists()
        ls.rm_mp, ls.rm_mp_cap, ls.erase_obs, ls.erase_cap, ls.rm_kf, ls.rm_kf_cap = p(lists[0]), len(rm_mp), p(lists[1]), len(erase), p(lists[2]), len(rm_kf)
        result, dead = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(NMP, dtype=torch.int32, device="cuda")
        o = _lib.gl_map_remove_out()
        o.result, o.dead_mp, o.dead_cap = p(result), p(dead), NMP
        tr = event_us(lambda: ctx.lib.gl_map_remove(ctx.h, NMP, NKF, NFK, NOBS, ref_(ed), p(rs.bd["kf_uvr"]), int(ba["kf_first"]), ref_(ls), ref_(o)), rs.restore, REPS)
        nobs, n_dead, _ = result.tolist()
        res[name] = {"NMP": NMP, "NKF": NKF, "NFK": NFK, "NOBS": NOBS, "candidates": len(sc["cand"]), "culled": n_cull,
                     "cull_device_us_median_min_max": tc, "removed": [len(rm_mp), len(erase), len(rm_kf)], "nobs_after": nobs, "dead": n_dead,
                     "remove_device_us_median_min_max": tr, "equal_to_restatement": bool(same)}
    print(json.dumps(res))


def pass_legs():
    sc = scene("euroc")
    m, ba = sc["m"], sc["ba"]
    NMP, NKF, NFK, NOBS = R._sizes(m)
    kf_row = int(sc["cand"][5])
    _, erase, _ = ES.removals(sc, 3, erase_frac=0.0002)
    row = torch.tensor([kf_row], dtype=torch.int32, device="cuda")
    res = {"mode": MODE, "lib": os.path.basename(os.path.dirname(os.path.abspath(os.environ.get("GMMLOC_HIP_LIB", "gmmloc_amd/x")))), "reps": REPS,
           "NMP": NMP, "NKF": NKF, "NFK": NFK, "NOBS": NOBS, "n_erase": len(erase)}
    rs = Resident(sc)
    if MODE == "device":
        depth = T(sc["kf_depth"])
        er = T(erase)
        out = {}

        def call():
            e = api.map_remove(ctx, rs.md, rs.bd, erase_obs=er, mp_ref_kf=rs.ref_kf)
            conn = api.update_connections(ctx, e["map"], row, Ccap=64)
            c = api.cull_keyframes(ctx, e["map"], e["ba"], depth, sc["th_depth"], conn["conn_kf"], conn["n_conn"])
            out["k"] = api.map_remove(ctx, e["map"], e["ba"], rm_kf=c["cull_rows"][0], n_rm_kf=c["n_cull"], mp_ref_kf=rs.ref_kf)
            out["c"], out["e"] = c, e
        res["host_to_host_us_median_min_max"] = wall_us(call, rs.restore, REPS)
        res.update(culled=int(out["c"]["n_cull"][0]), nobs_after=out["k"]["nobs"], dead=out["e"]["n_dead"] + out["k"]["n_dead"], bytes_up=4 * len(erase), bytes_down=24)
    elif MODE == "upload":
        keys = MUTABLE + ("obs_feat",)
        host = {k: torch.from_numpy(np.ascontiguousarray(m[k] if k in m else ba[k])).pin_memory() for k in keys}
        tgt = {k: (rs.md[k] if k in rs.md else rs.bd[k]) for k in keys}
        out = {}

        def call():
            for k in keys:  # the host's rows after its own erase
                tgt[k].copy_(host[k], non_blocking=True)
            out["conn"] = api.update_connections(ctx, rs.md, row, Ccap=64)
            out["n"] = out["conn"]["n_conn"].tolist()  # the list back: the host culls on it
            for k in keys:  # ... and after its own cull
                tgt[k].copy_(host[k], non_blocking=True)
        res["host_to_host_us_median_min_max"] = wall_us(call, lambda: None, REPS)
        res.update(bytes_up=int(2 * sum(v.numel() * v.element_size() for v in host.values())), bytes_down=4)
    else:
        raise SystemExit("mode: kernels | device | upload | all")
    print(json.dumps(res))


if __name__ == "__main__":
    if MODE == "kernels":
        kernels_leg()
    else:
        pass_legs()
