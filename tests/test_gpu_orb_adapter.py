"""The C++ host mirror's orbDescribe (include/gmmloc_hip/gmm_adapter.hpp) must give what the Python host gives through the same C-ABI:
a g++-built driver (tests/cpp/orb_check.cpp) takes a random scene of tests/orb_scenes.py as host vectors and bordered level images;
its outputs equal the Python host's (and the model's) bit for bit."""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import cpp_driver, orb_dev, orb_scenes
from tests.gpu_helpers import stop_on_device_error  # noqa: F401 (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
ROW_PAD = 38  # bytes behind every row: EDGE_THRESHOLD = 19 on both sides


@pytest.mark.parametrize("angles", [False, True], ids=["orientation computed", "kp_angle given"])
def test_cpp_orb_describe_matches_python_host(gpu, map_v1, tmp_path, angles):
    torch, ctx = gpu
    exe = cpp_driver.build("orb_check", tmp_path)
    api.GMM(ctx, *map_v1).save(tmp_path / "m.gmm")  # (the adapter's object is a loaded model; the call does not read it)
    scene = orb_scenes.random_scene(2, angles=angles)
    N = len(scene["kp_oct"])
    with open(tmp_path / "scene.bin", "wb") as fh:
        np.array([N, len(scene["levels"]), ROW_PAD, int(angles)], np.int32).tofile(fh)
        np.array(scene["blur_w"], np.int32).tofile(fh)
        np.array([scene["scale_factor"]], np.float64).tofile(fh)
        scene["kp_xy"].tofile(fh)
        scene["kp_oct"].tofile(fh)
        if angles:
            scene["kp_angle"].tofile(fh)
        scene["pattern"].tofile(fh)
        for im in scene["levels"]:
            np.array([im.shape[1], im.shape[0]], np.int32).tofile(fh)
            np.pad(im, ((0, 0), (0, ROW_PAD)), constant_values=0xEE).tofile(fh)
    r = cpp_driver.run(exe, tmp_path / "m.gmm", tmp_path / "scene.bin", tmp_path / "out.bin")
    assert r.returncode == 0, r.stderr
    got = {}
    with open(tmp_path / "out.bin", "rb") as fh:
        for k, dt, shape in (("desc", np.uint8, (1, N, 32)), ("angle", np.float32, (1, N)), ("moments", np.int32, (1, N, 2)),
                             ("uv32", np.float32, (1, N, 2)), ("uv64", np.float64, (1, N, 2)), ("stat", np.int32, (1, 2))):
            got[k] = np.fromfile(fh, dt, int(np.prod(shape))).reshape(shape)
        assert fh.read() == b""
    host = orb_dev.run(torch, ctx, [scene], scene["pattern"], scene["blur_w"], scene["scale_factor"])
    assert host["stat"][0, 0] > 100
    orb_dev.same_bits(got, host, "the C++ host against the Python host")
    orb_dev.same_bits(host, orb_dev.expected([orb_scenes.model_of(("adapter", angles), scene)], N), "the Python host against the model")
