"""The C++ host mirror's computeStereoMatches (include/gmmloc_hip/gmm_adapter.hpp) must give what the Python host gives through the same
C-ABI: a g++-built driver (tests/cpp/stereo_check.cpp) takes a random scene of tests/stereo_scenes.py as host vectors and bordered level
images; its outputs equal the Python host's (and the model's) bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import cpp_driver, stereo_dev, stereo_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
ROW_PAD = 38  # bytes behind every row: EDGE_THRESHOLD = 19 on both sides


def test_cpp_stereo_matches_python_host(gpu, map_v1, tmp_path):
    torch, ctx = gpu
    exe = cpp_driver.build("stereo_check", tmp_path)
    api.GMM(ctx, *map_v1).save(tmp_path / "m.gmm")  # (the adapter's object is a loaded model; the call does not read it)
    scene = stereo_scenes.random_scene(2)
    f, cam = scene["frame"], scene["cam"]
    NF, NR = len(f["feat_oct"]), len(f["r_oct"])
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([NF, NR, len(f["pyr_left"]), cam[2], ROW_PAD], np.int32).tofile(fh)
        np.array([cam[0], cam[1], scene["scale_factor"]], np.float64).tofile(fh)
        for k in ("feat_uv", "feat_oct", "feat_desc", "r_uv", "r_oct", "r_desc"):
            np.ascontiguousarray(f[k]).tofile(fh)
        for side in ("pyr_left", "pyr_right"):
            for im in f[side]:
                np.array([im.shape[1], im.shape[0]], np.int32).tofile(fh)
                np.pad(im, ((0, 0), (0, ROW_PAD)), constant_values=0xEE).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    got = {}
    with open(tmp_path / "out.bin", "rb") as fh:
        for k, dt, n in (("feat_ur", np.float32, NF), ("feat_depth", np.float32, NF), ("match_r", np.int32, NF), ("sad", np.int32, NF),
                         ("stat", np.int32, 4)):
            got[k] = np.fromfile(fh, dt, n).reshape((1, n))
        assert fh.read() == b""
    host = stereo_dev.run(torch, ctx, cam, scene["scale_factor"], [f])
    assert host["stat"][0, 1] > 50
    stereo_dev.same_bits(got, host, "the C++ host against the Python host")
    stereo_dev.same_bits(host, stereo_dev.expected([stereo_scenes.model_of(("random", 2), scene)], NF), "the Python host against the model")
