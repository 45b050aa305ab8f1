"""gl_orb_describe on a list of images of the model's form (tests/orb_ref.py): upload, pad, call, guard words, read back - stated once
for the GPU test modules of the call.  Test infrastructure; nothing in the product imports it."""
import numpy as np

OUT = {"desc": ("uint8", 32, 0), "angle": ("float32", None, -1.0), "moments": ("int32", 2, 0), "uv32": ("float32", 2, -1.0),
       "uv64": ("float64", 2, -1.0)}  # name -> dtype, trailing extent, the value of a skipped or padding slot
OUT_KEYS = tuple(OUT) + ("stat",)
GUARD = 64  # elements behind every output
_GUARD = {"uint8": 0xA5, "int32": -77077, "float32": -77.25, "float64": -77.25}


def pack(items, N=None):
    """the images' key-points as one batch of N slots.  Slots at or beyond an image's count are padding that WOULD be described if it
    were read: copies of the image's own key-points."""
    B = len(items)
    ns = [len(it["kp_oct"]) for it in items]
    N = max(ns) if N is None else N
    angles = items[0].get("kp_angle") is not None
    a = dict(kp_xy=np.full((B, N, 2), 19, np.int32), kp_oct=np.zeros((B, N), np.int32),
             n_kp=np.array([n if it.get("n_kp") is None else it["n_kp"] for it, n in zip(items, ns)], np.int32))
    if angles:
        a["kp_angle"] = np.zeros((B, N), np.float32)
    for b, (it, n) in enumerate(zip(items, ns)):
        assert (it.get("kp_angle") is not None) == angles, "one batch: kp_angle for every image or for none"
        for k in ("kp_xy", "kp_oct") + (("kp_angle",) if angles else ()):
            a[k][b, :n] = it[k]
            if n and N > n:
                a[k][b, n:] = it[k][np.arange(N - n) % n]
    return a, N


def expected(outs, N):
    """the model's per-image outputs stacked, padded to N slots"""
    r = {"stat": np.stack([o["stat"] for o in outs])}
    for k, (dt, trail, fill) in OUT.items():
        r[k] = np.full((len(outs), N) + ((trail,) if trail else ()), fill, dt)
        for b, o in enumerate(outs):
            r[k][b, :len(o[k])] = o[k]
    return r


def guarded(torch, shape, dtype, dev):
    """an output of that shape with GUARD elements behind it -> (the view the call gets, the whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), _GUARD[dtype], dtype=getattr(torch, dtype), device=dev)
    return whole[:n].view(*shape), whole


def run(torch, ctx, items, pattern, blur_w, scale_factor=1.2, N=None, row_pad=0, lead=0, counts=True):
    """-> the call's outputs as numpy arrays.  Asserts on the way: the guard words behind every output are intact and no input byte
    (key-points, counts, pattern, pyramid) has changed.  counts=False: n_kp is not passed (NULL: all slots)."""
    from gmmloc_amd import orb, stereo
    a, N = pack(items, N)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    pat = torch.from_numpy(np.ascontiguousarray(pattern)).to(dev)
    pyr = stereo.Pyramid([it["levels"] for it in items], dev, row_pad=row_pad, lead=lead, fill=0xAB)
    pyr_before = pyr.data.cpu().numpy().copy()
    B = len(items)
    out, whole = {}, {}
    for k, (dt, trail, _) in OUT.items():
        out[k], whole[k] = guarded(torch, (B, N) + ((trail,) if trail else ()), dt, dev)
    out["stat"], whole["stat"] = guarded(torch, (B, 2), "int32", dev)
    orb.describe(ctx, t["kp_xy"], t["kp_oct"], pat, pyr, blur_w=blur_w, scale_factor=scale_factor, n_kp=t["n_kp"] if counts else None,
                 kp_angle=t.get("kp_angle"), out=out)
    ctx.synchronize()
    got = {k: out[k].cpu().numpy() for k in OUT_KEYS}
    for k in OUT_KEYS:
        tail = whole[k][-GUARD:].cpu().numpy()
        assert np.all(tail == tail.dtype.type(_GUARD[str(tail.dtype)])), "guard words behind %s overwritten" % k
    for k, v in a.items():
        assert np.array_equal(t[k].cpu().numpy().view(np.uint8), v.view(np.uint8)), "input %s changed" % k
    assert np.array_equal(pat.cpu().numpy(), pattern), "the pattern changed"
    assert np.array_equal(pyr.data.cpu().numpy(), pyr_before), "the pyramid changed"
    return got


def same_bits(got, ref, label):
    """every output equal, floats by their bits"""
    for k in OUT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)  # (empty when only a zero's sign or a NaN's payload differs)
            first = tuple(bad[0]) if len(bad) else ()
            raise AssertionError("%s, output %s: %d of %d elements differ, first at %s: device %r, expected %r" %
                                 (label, k, len(bad), a.size, first, a[first] if first else None, b[first] if first else None))
