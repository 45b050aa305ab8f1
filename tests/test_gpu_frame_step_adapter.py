"""The C++ host mirror's endFrame, noteReplaced and nextFrame (include/gmmloc_hip/gmm_adapter.hpp) must give what the Python host gives
through the same C-ABI: a g++-built driver (tests/cpp/frame_step_check.cpp) keeps the map of tests/frame_step_cases.py::after_map on
the device, ends the four frames of END, notes the steps of REPLACE['all'] and hands the frames of NEXT over with that array; every
output it downloads is compared bit for bit with frame_step.frame_end / note_replaced / frame_next on the same bytes - and with the
declared outputs of the cases."""
import numpy as np
import pytest

from gmmloc_amd import api, frame_step
from tests import cpp_driver
from tests import frame_step_cases as FC
from tests.test_frame_step_cases import check_next_rows, next_args, poison_end
from tests.gpu_helpers import to_dev
from tests.test_gpu_frame_step import device_next, host, map_dev

pytestmark = pytest.mark.gpu


def test_cpp_frame_step_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    mean, cov = map_v1
    exe = cpp_driver.build("frame_step_check", tmp_path)
    api.GMM(ctx, mean, cov).save(tmp_path / "m.gmm")
    m, ba, tracked, prev, ref_kf2, held = next_args()  # (after_map)
    NMP, (NKF, NFK), NOBS = len(m["mp_valid"]), m["kf_mp"].shape, len(m["obs_kf"])
    a = FC.end_arrays()
    B, NF = a["feat_mp"].shape
    NL, NPcap = a["last_observed"].shape[1], a["local_mp"].shape[1]
    steps = FC.REPLACE["all"][0]
    src, tgt = np.array([s for s, _ in steps], np.int32), np.array([t for _, t in steps], np.int32)
    fn = np.array([FC.NEXT_FEAT_NEW] * 2, np.int32)
    rule = frame_step.kf_rule(**FC.END_RULE)
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NMP, NKF, NFK, NOBS, FC.NMPCAP, B, NF, NL, NPcap, len(steps), held.shape[0], held.shape[1], FC.NEXT_MP_BASE, 0, 0, 0], np.int32).tofile(fh)
        for arr in (m["mp_valid"], m["kf_valid"], m["kf_mp"], m["obs_ptr"], m["obs_kf"], ba["obs_feat"], ba["kf_uvr"], ba["kf_oct"], ba["kf_pose"], m["mp_pos"],
                    m["mp_desc"], a["feat_mp"], a["match_last"], a["match_local"], a["outlier"], a["local_mp"], a["n_local_mp"], a["counts2"], a["ref_kf"],
                    a["last_observed"], a["feat_depth"], np.array([FC.TH_DEPTH], np.float32)):
            np.ascontiguousarray(arr).tofile(fh)
        fh.write(bytes(rule))
        for arr in (src, tgt, tracked, prev, ref_kf2, held, fn):
            np.ascontiguousarray(arr).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    # the same sequence from Python on the same bytes
    md, bd = map_dev(torch, m, ba)
    d = to_dev(torch, a)
    end = frame_step.frame_end(ctx, md, bd, d, d, d["feat_depth"], FC.TH_DEPTH, last_observed=d["last_observed"], rule=rule,
                               out=to_dev(torch, poison_end(B, NF)))
    rep = torch.full((FC.NMPCAP,), -1, dtype=torch.int32).cuda()
    frame_step.note_replaced(ctx, rep, torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda())
    torch.cuda.synchronize()
    B2, NF2 = held.shape
    f = lambda *s, dt=np.float64, v=-77.0: np.full(s, v, dt)
    outs = dict(t_rc=f(B2, 7), t_cr=f(B2, 7), pose_lw=f(B2, 7), pose_cw=f(B2, 7), last_pt=f(B2, NF2, 3), last_valid=f(B2, NF2, dt=np.uint8, v=77),
                last_observed=f(B2, NF2, dt=np.uint8, v=77), held=f(B2, NF2, dt=np.uint8, v=77), status=f(B2, dt=np.int32, v=-77),
                last_desc=f(B2, NF2, 32, dt=np.uint8, v=77))
    nxt = device_next(torch, ctx, md, bd, tracked, prev, ref_kf2, held, feat_new=fn, mp_base=FC.NEXT_MP_BASE, mp_replaced=rep.cpu().numpy(), poison=outs)
    end = host(end)
    assert np.array_equal(rep.cpu().numpy(), FC.replaced_array("all"))
    check_next_rows(m, nxt, FC.NEXT_OUT)
    assert end["stat"][1].tolist() == [0, 10, 0, 0, 0, 0, 0, 0] and (end["held_mp"][1] == -77).all() and end["stat"][0, 1] > 0
    out = open(tmp_path / "out.bin", "rb")
    rd = lambda dt, cnt: np.fromfile(out, dt, cnt)
    for name, arr in (("held_mp", end["held_mp"]), ("held", end["held"]), ("stat", end["stat"]), ("ratio_map", end["ratio_map"]), ("mp_replaced", rep.cpu().numpy()),
                      ("t_rc", nxt["t_rc"]), ("t_cr", nxt["t_cr"]), ("pose_lw", nxt["pose_lw"]), ("pose_cw", nxt["pose_cw"]), ("held_mp2", nxt["held_mp"]),
                      ("last_pt", nxt["last_pt"]), ("last_valid", nxt["last_valid"]), ("last_observed", nxt["last_observed"]), ("held2", nxt["held"]),
                      ("status", nxt["status"]), ("last_desc", nxt["last_desc"])):
        assert rd(arr.dtype, arr.size).tobytes() == np.ascontiguousarray(arr).tobytes(), name
    assert out.read() == b""
