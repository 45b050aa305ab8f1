"""The scenes of tests/test_map_edit_ref.py (CPU: the conditions that keep the GPU tests from passing vacuously) and
tests/test_gpu_map_edit.py (GPU: gl_cull_keyframes / gl_map_remove against tests/map_edit_ref.py): the maps of
tests/ba_window_scenes.py with what the culling reads added, pinned seeds.  Test infrastructure; nothing in the product imports it."""
import numpy as np

from tests import ba_window_scenes as S

TH_DEPTH = 6.0
CLAMP = {"small": 1, "tiny": 2}  # the octaves clamped so that most observations meet the scale condition: key-frames get culled
NCAND = 40


def first_entry_kf(m):
    """mp_ref_kf as a fresh map has it: the key-frame of every point's first CSR entry (-1 without one)"""
    ptr, okf = np.asarray(m["obs_ptr"]).astype(np.int64), np.asarray(m["obs_kf"])
    NOBS = len(okf)
    has = (ptr[:-1] >= 0) & (ptr[1:] > ptr[:-1]) & (ptr[1:] <= NOBS)
    return np.where(has, okf[np.clip(ptr[:-1], 0, max(NOBS - 1, 0))] if NOBS else -1, -1).astype(np.int32)


def scene(name, clamp=False):
    """-> dict(m, ba, rows, kf_depth (NKF,NFK) f32: uniform 0.2 - 8 m, -1 where u_right < 0; th_depth; cand: the first NCAND valid rows;
    mp_ref_kf).  clamp: the variant with kf_oct = minimum(kf_oct, CLAMP[name])."""
    m, ba, rows = S.scene(name)
    seed = S.SCENES[name][0]
    rng = np.random.default_rng(seed + 777)
    depth = rng.uniform(0.2, 8.0, ba["kf_oct"].shape).astype(np.float32)
    depth[ba["kf_uvr"][:, :, 2] < 0] = -1.0
    if clamp:
        ba["kf_oct"] = np.minimum(ba["kf_oct"], CLAMP[name]).astype(np.int32)
    cand = np.nonzero(m["kf_valid"])[0][:NCAND].astype(np.int32)
    return dict(m=m, ba=ba, rows=rows, kf_depth=depth, th_depth=TH_DEPTH, cand=cand, mp_ref_kf=first_entry_kf(m))


def removals(sc, seed, n_mp=20, n_kf=8, erase_frac=0.03):
    """a set of removals of the three kinds on a scene -> (rm_mp, erase_obs ascending, rm_kf in a random order); with a duplicate, an
    invalid and an out-of-range entry in each list when `dirty`"""
    m, ba = sc["m"], sc["ba"]
    rng = np.random.default_rng(seed)
    NMP, NKF, NOBS = len(m["mp_valid"]), len(m["kf_valid"]), len(m["obs_kf"])
    rm_mp = rng.choice(np.nonzero(m["mp_valid"])[0], min(n_mp, NMP // 4), replace=False).astype(np.int32)
    erase = np.sort(rng.choice(NOBS, max(int(NOBS * erase_frac), 3), replace=False)).astype(np.int32)
    ok = np.nonzero(m["kf_valid"])[0]
    ok = ok[ok != ba["kf_first"]]
    rm_kf = rng.choice(ok, min(n_kf, len(ok) // 2), replace=False).astype(np.int32)
    return rm_mp, erase, rm_kf


def dirty(sc, rm_mp, erase, rm_kf):
    """the same lists with entries that change nothing: a duplicate, an invalid row, rows outside the tables, kf_first"""
    m, ba = sc["m"], sc["ba"]
    NMP, NKF, NOBS = len(m["mp_valid"]), len(m["kf_valid"]), len(m["obs_kf"])
    bad_mp = np.nonzero(m["mp_valid"] == 0)[0][:1]
    bad_kf = np.nonzero(m["kf_valid"] == 0)[0][:1]
    rm_mp = np.concatenate([rm_mp[:1], [-1, NMP], bad_mp, rm_mp, rm_mp[:2]]).astype(np.int32)
    erase = np.concatenate([[-5], erase, [NOBS, 2 ** 31 - 1], erase[:2]]).astype(np.int32)
    rm_kf = np.concatenate([rm_kf[:2], [ba["kf_first"], -1, NKF], bad_kf, rm_kf[2:], rm_kf[:1]]).astype(np.int32)
    return rm_mp, erase, rm_kf
