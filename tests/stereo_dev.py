"""gl_stereo_matches on a list of frames of the model's form (tests/stereo_ref.py): upload, pad, call, guard words, read back - stated once
for the GPU test modules of the stereo matcher.  Test infrastructure; nothing in the product imports it."""
import numpy as np

OUT_KEYS = ("feat_ur", "feat_depth", "match_r", "sad", "stat")
GUARD = 64  # elements behind every output
_F32_GUARD, _I32_GUARD = np.float32(-77.25), np.int32(-77077)


def pack(frames, NF=None, NR=None, seed=5):
    """the frames as one batch of NF x NR slots: numpy arrays of the call's inputs.  Slots at or beyond a frame's count are padding
    that WOULD match if it were read: copies of the frame's own key-points (of its first one; zeros in an empty frame)."""
    B = len(frames)
    nl = [len(f["feat_oct"]) for f in frames]
    nr = [len(f["r_oct"]) for f in frames]
    NF, NR = max(nl) if NF is None else NF, max(nr) if NR is None else NR
    a = dict(feat_uv=np.zeros((B, NF, 2)), feat_oct=np.zeros((B, NF), np.int32), feat_desc=np.zeros((B, NF, 32), np.uint8),
             r_uv=np.zeros((B, NR, 2), np.float32), r_oct=np.zeros((B, NR), np.int32), r_desc=np.zeros((B, NR, 32), np.uint8),
             n_left=np.array([f.get("n_left", n) if f.get("n_left") is not None else n for f, n in zip(frames, nl)], np.int32),
             n_right=np.array([f.get("n_right", n) if f.get("n_right") is not None else n for f, n in zip(frames, nr)], np.int32))
    for b, f in enumerate(frames):
        for keys, n, N in ((("feat_uv", "feat_oct", "feat_desc"), nl[b], NF), (("r_uv", "r_oct", "r_desc"), nr[b], NR)):
            for k in keys:
                a[k][b, :n] = f[k]
                if n and N > n:
                    a[k][b, n:] = f[k][np.arange(N - n) % n]
    return a, NF, NR


def expected(outs, NF):
    """the model's per-frame outputs stacked, padded to NF slots with -1"""
    r = {}
    for k in OUT_KEYS:
        if k == "stat":
            r[k] = np.stack([o[k] for o in outs])
        else:
            r[k] = np.full((len(outs), NF), -1, outs[0][k].dtype)
            for b, o in enumerate(outs):
                r[k][b, :len(o[k])] = o[k]
    return r


def guarded(torch, shape, dtype, dev):
    """an output of that shape with GUARD words behind it -> (the view the call gets, the whole buffer)"""
    n = int(np.prod(shape))
    fill = float(_F32_GUARD) if dtype == torch.float32 else int(_I32_GUARD)
    whole = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return whole[:n].view(*shape), whole


def run(torch, ctx, cam, scale_factor, frames, NF=None, NR=None, row_pad=0, lead=0, counts=True):
    """-> the call's outputs as numpy arrays.  Asserts on the way: the guard words behind every output are intact and no input byte
    (features, key-points, counts, pyramids) has changed.  counts=False: n_left / n_right are not passed (NULL: all slots)."""
    from gmmloc_amd import api, stereo
    a, NF, NR = pack(frames, NF, NR)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    pl = stereo.Pyramid([f["pyr_left"] for f in frames], dev, row_pad=row_pad, lead=lead, fill=0xAB)
    pr = stereo.Pyramid([f["pyr_right"] for f in frames], dev, row_pad=row_pad, lead=lead, fill=0xCD)
    pyr_before = [pl.data.cpu().numpy().copy(), pr.data.cpu().numpy().copy()]
    B = len(frames)
    out, whole = {}, {}
    for k in OUT_KEYS:
        shape = (B, 4) if k == "stat" else (B, NF)
        out[k], whole[k] = guarded(torch, shape, torch.float32 if k in ("feat_ur", "feat_depth") else torch.int32, dev)
    left = {k: t[k] for k in ("feat_uv", "feat_oct", "feat_desc")}
    right = {k: t[k] for k in ("r_uv", "r_oct", "r_desc")}
    if counts:
        left["n_left"], right["n_right"] = t["n_left"], t["n_right"]
    c = api.Camera(fx=cam[0], fy=cam[0], bf=cam[1], height=int(cam[2]))
    stereo.stereo_matches(ctx, c, left, right, pl, pr, scale_factor=scale_factor, out=out)
    ctx.synchronize()
    got = {k: out[k].cpu().numpy() for k in OUT_KEYS}
    for k in OUT_KEYS:
        tail = whole[k][-GUARD:].cpu().numpy()
        assert np.all(tail == (_F32_GUARD if tail.dtype == np.float32 else _I32_GUARD)), "guard words behind %s overwritten" % k
    for k, v in a.items():
        assert np.array_equal(t[k].cpu().numpy().view(np.uint8), v.view(np.uint8)), "input %s changed" % k
    assert np.array_equal(pl.data.cpu().numpy(), pyr_before[0]) and np.array_equal(pr.data.cpu().numpy(), pyr_before[1]), "a pyramid changed"
    return got


def same_bits(got, ref, label):
    """np.array_equal on every output, floats by their bits"""
    for k in OUT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a.view(np.int32), b.view(np.int32)):
            bad = np.argwhere(a.view(np.int32) != b.view(np.int32))
            raise AssertionError("%s, output %s: %d of %d elements differ, first at %s: device %r, expected %r" %
                                 (label, k, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))
