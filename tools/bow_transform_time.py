#!/usr/bin/env python3
"""Times of the DBoW2 transform on the device (gl_bow_transform), one JSON line per run, on synth_vocabulary(10, 6) - the shape of the
ORB vocabulary, 1 111 110 records - and frames of 1 200 descriptors drawn near node descriptors, levelsup = 4:
    python tools/bow_transform_time.py calls [reps]    device time of the whole call (HIP events around calls enqueued back to back),
                                                       B = 1 and B = 64 frames of 1 200 features
    python tools/bow_transform_time.py kernels         a few calls of either shape, for `rocprofv3 --kernel-trace --stats` (the descent and
                                                       the CSR kernel separately)
    python tools/bow_transform_time.py a|b [reps]      ONE key-frame's feature-vector row of the resident tables (1 200 features,
                                                       NNcap = 1 200), host to host - the wall clock around work that ends in a synchronise:
       a  the row made on the device: transform_into_tables on the descriptors that are resident already, one synchronise
       b  the route of the parent commit: the row ready-made on the host (its own transform NOT priced: the host's DBoW2 and its
          dependencies are no part of this project) copied into the tables from page-locked memory, one synchronise
    python tools/bow_transform_time.py run [reps]      calls, kernels under rocprofv3, then a and b alternated three times, EACH RUN A
                                                       PROCESS OF ITS OWN under its own time limit, stopping at the first failure; prints
                                                       every line and the verdict on the two legs' intervals (min .. max of three medians).
No number is promised and none is compared with the host's DBoW2, which cannot be measured here: leg b is an upload alone."""
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODE = sys.argv[1] if len(sys.argv) > 1 else "run"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
NF, NN, LEVELSUP = 1200, 1200, 4


def orchestrate():
    def child(mode, limit, prefix=()):
        r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__), mode, str(REPS)], cwd=ROOT, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            print("FAILED %s (exit %d), nothing more is started:\n%s" % (mode, r.returncode, (r.stderr or r.stdout)[-2000:]))
            raise SystemExit(1)
        d = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
        print(json.dumps(d))
        sys.stdout.flush()
        return d
    child("calls", 300)
    out = os.path.join(ROOT, "build_tmp", "bow_prof")  # (ignored by git, like the *.db it holds)
    child("kernels", 420, ("rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "bow", "--"))
    dbs = sorted(glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True))
    if dbs:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocpd_summary.py"), dbs[-1]], capture_output=True, text=True, timeout=120)
        print("rocprofv3 --kernel-trace --stats, the transform's kernels (20 calls of B = 1, grid 75x1 / 1, then 20 of B = 64, grid 75x64 / 64):")
        # per launch shape only name, grid, calls and times: registers and LDS are the code object's (tools/kernel_meta.py)
        def shape_line(ln):
            f = ln.split()
            if "grid x wg" in ln:
                f = ["kernel", "grid x wg", "calls", "total_us", "avg_us"]
            elif len(f) < 5 or "/" not in f[1]:
                return ln
            return "%-50s %14s %6s %12s %12s" % tuple(f[:5])
        print("\n".join(shape_line(ln) for ln in r.stdout.splitlines() if "k_bow" in ln or ln.startswith("kernel")))
    else:
        print("no rocprofv3 result found under %s: the kernels are not priced separately" % out)
    med = {"a": [], "b": []}
    for _ in range(3):
        for leg in ("a", "b"):
            med[leg].append(child(leg, 240)["host_to_host_us_median_min_max"][0])
    ia, ib = (min(med["a"]), max(med["a"])), (min(med["b"]), max(med["b"]))
    print("one key-frame's feature-vector row, host to host, us, the three medians per leg: a (made on the device) %s  b (uploaded ready-made) %s" %
          (" ".join("%.1f" % v for v in med["a"]), " ".join("%.1f" % v for v in med["b"])))
    if ia[1] < ib[0]:
        print("the intervals do not overlap: a %.1f .. %.1f us < b %.1f .. %.1f us" % (ia + ib))
    else:
        print("the intervals overlap or a is slower (a %.1f .. %.1f us, b %.1f .. %.1f us): the resident route is NOT faster host to host than an "
              "upload whose transform is not priced; what it removes is the host's transform and %d bytes of upload per key-frame" %
              (ia + ib + (4 * (1 + NN + NN + 1 + NF),)))


if MODE == "run":
    orchestrate()
    raise SystemExit(0)

import torch  # noqa: E402

import gmmloc_amd  # noqa: E402
from gmmloc_amd import bow, synth  # noqa: E402

ctx = gmmloc_amd.Context(0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
voc_h = synth.synth_vocabulary(10, 6, 14)
voc = bow.Vocabulary.from_arrays(ctx, voc_h["parent"], voc_h["desc"], voc_h["weight"], voc_h["is_leaf"], 10, 6)


def frames(B):
    return T(np.stack([synth.synth_vocabulary_descriptors(voc_h, NF, 100 + b) for b in range(B)]))


def events_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ctx.stream):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0.record(ctx.stream)
        for _ in range(n):
            fn()
        e1.record(ctx.stream)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def med3(fn, n=50):
    ts = [events_us(fn, n) for _ in range(max(REPS // 4, 5))]
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def shapes():
    for B in (1, 64):
        d = frames(B)
        out = bow.transform(ctx, voc, d, None, levelsup=LEVELSUP, nn_cap=NN)
        torch.cuda.synchronize()
        yield B, d, out


def calls():
    res = {"mode": "calls", "device": torch.cuda.get_device_name(0), "reps": REPS, "vocabulary": voc.info()}
    for B, d, out in shapes():
        res["transform_b%d_nf%d_device_us_median_min_max" % (B, NF)] = med3(lambda: bow.transform(ctx, voc, d, None, levelsup=LEVELSUP, out=out))
        res["b%d_nodes_kept_of_frame_0" % B] = [int(out["nnode"][0]), int(out["node_ptr"][0, int(out["nnode"][0])])]
    print(json.dumps(res))


def kernels():
    for B, d, out in shapes():
        for _ in range(20):
            bow.transform(ctx, voc, d, None, levelsup=LEVELSUP, out=out)
        torch.cuda.synchronize()
    print(json.dumps({"mode": "kernels", "calls_per_shape": 21}))


def wall_us(fn, n):
    ts = []
    with torch.cuda.stream(ctx.stream):
        for i in range(n + 10):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if i >= 10:
                ts.append(1e6 * (time.perf_counter() - t))
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def leg(which):
    NKF, row = 8, 5
    tables = dict(desc=frames(NKF), **bow.feature_vector_alloc(NKF, NF, NN))
    res = {"mode": which, "reps": REPS}
    if which == "a":
        def call():
            bow.transform_into_tables(ctx, voc, tables, row, levelsup=LEVELSUP)
            torch.cuda.synchronize()
    else:
        r = bow.transform(ctx, voc, tables["desc"][row:row + 1], None, levelsup=LEVELSUP, nn_cap=NN, per_feature=False)
        torch.cuda.synchronize()
        pinned = {k: r[k].cpu().pin_memory() for k in bow.FV_KEYS}  # the row as the host's own transform would hand it over
        res["bytes_uploaded"] = int(sum(t.numel() * 4 for t in pinned.values()))

        def call():
            for k, h in pinned.items():
                tables[k][row:row + 1].copy_(h, non_blocking=True)
            torch.cuda.synchronize()
    res["host_to_host_us_median_min_max"] = wall_us(call, REPS)
    print(json.dumps(res))


if MODE == "calls":
    calls()
elif MODE == "kernels":
    kernels()
elif MODE in ("a", "b"):
    leg(MODE)
else:
    raise SystemExit("mode: run | calls | kernels | a | b")
