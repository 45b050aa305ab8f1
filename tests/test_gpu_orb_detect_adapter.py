"""The C++ host mirror's orbPyramid / orbDetect / orbExtract (include/gmmloc_hip/gmm_adapter.hpp) must give what the Python host gives
through the same C-ABI: a g++-built driver (tests/cpp/orb_detect_check.cpp) takes a random image of tests/orb_detect_dev.py with padded
rows; its levels, key-points and descriptors equal the Python host's and the model's bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import cpp_driver, orb_detect_dev as dev, orb_detect_ref as ref, orb_ref, orb_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
ROW_PAD, NLEVELS, NFEATURES, CAP = 11, 4, 250, 2048


def test_cpp_orb_front_matches_python_host_and_model(gpu, map_v1, tmp_path):
    from gmmloc_amd import orb
    torch, ctx = gpu
    exe = cpp_driver.build("orb_detect_check", tmp_path)
    api.GMM(ctx, *map_v1).save(tmp_path / "m.gmm")  # (the adapter's object is a loaded model; the calls do not read it)
    image = dev.scene(41, (200, 150))
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([200, 150, ROW_PAD, NLEVELS, NFEATURES, 20, 7, CAP], np.int32).tofile(fh)
        orb_scenes.PATTERN.tofile(fh)
        np.pad(image, ((0, 0), (0, ROW_PAD)), constant_values=0xEE).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    levels = ref.pyramid(image, NLEVELS)
    m = ref.detect(levels, NFEATURES, cand_cap=CAP)
    n = len(m["kp_oct"])
    assert n > 150
    want = orb_ref.describe(levels, m["kp_xy"], m["kp_oct"], orb_scenes.PATTERN, orb_ref.default_blur(2.0))
    assert all(orb_ref.trig_margin_ok(v) for v in want["angle"] if v >= 0)
    d = torch.device("cuda:0")
    _, det, des = orb.extract(ctx, torch.from_numpy(image[None]).to(d), torch.from_numpy(orb_scenes.PATTERN).to(d), nfeatures=NFEATURES,
                              nlevels=NLEVELS, cand_cap=CAP)
    ctx.synchronize()
    with open(tmp_path / "out.bin", "rb") as fh:
        for l, lv in enumerate(levels):
            assert list(np.fromfile(fh, np.int32, 2)) == [lv.shape[1], lv.shape[0]]
            assert np.array_equal(np.fromfile(fh, np.uint8, lv.size).reshape(lv.shape), lv), l
        for call in ("orbDetect", "orbExtract"):
            assert int(np.fromfile(fh, np.int32, 1)[0]) == n == int(det["n_kp"][0]), call
            assert np.array_equal(np.fromfile(fh, np.int32, 8), m["level_count"]) and np.array_equal(np.fromfile(fh, np.int32, 4), m["stat"]), call
            for k, dt, tr in (("kp_xy", np.int32, 2), ("kp_oct", np.int32, 1), ("kp_response", np.float32, 1)):
                got = np.fromfile(fh, dt, n * tr).reshape(m[k].shape)
                assert got.tobytes() == m[k].tobytes() == det[k][0, :n].cpu().numpy().tobytes(), (call, k)
        for k, dt, tr in (("desc", np.uint8, 32), ("angle", np.float32, 1), ("moments", np.int32, 2), ("uv32", np.float32, 2), ("uv64", np.float64, 2)):
            got = np.fromfile(fh, dt, n * tr).reshape(want[k].shape)
            assert got.tobytes() == want[k].tobytes() == des[k][0, :n].cpu().numpy().tobytes(), k
        assert np.array_equal(np.fromfile(fh, np.int32, 2), want["stat"])
        assert fh.read() == b""
