"""CPU: the C-ABI shared library loads, exports every symbol include/gmmloc_hip.h declares,
and its host-only logic (.gmm reader / writer, default parameters, error reporting) works.
No compute entry point is called here (there is no GPU and no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cpp_driver
from tests.conftest import ROOT, GOLDEN

@pytest.fixture(scope="module")
def lib():
    from gmmloc_amd import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gmmloc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 25
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, missing
    assert not lib._gl_missing, lib._gl_missing
    # and the python binding table covers the header
    assert names == set(lib._gl_signatures), names ^ set(lib._gl_signatures)


def test_config_table_names_exported_functions(lib):
    """the table next to gl_camera / gl_params (which fields and which scale_factor each entry point reads) speaks of functions
    the library exports, and of every exported function that takes a camera or parameters"""
    hdr = open(os.path.join(ROOT, "include", "gmmloc_hip.h")).read()
    rows = re.findall(r"^ \* (gl_[a-z0-9_]+) +\|([^|]*)\|([^|]*)\|", hdr, flags=re.M)
    assert len(rows) >= 25
    missing = [n for n, _, _ in rows if not hasattr(lib, n)]
    assert not missing, missing
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    takes = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\([^;]*?const gl_(?:camera|params)\*", code))
    assert takes and takes <= {n for n, _, _ in rows}, takes - {n for n, _, _ in rows}


def test_default_params_match_reference_config(lib):
    from gmmloc_amd import api
    p = api.Params()
    c = p.c()
    assert c.neighbor_dist_thresh == 2.5 and c.tri_lambda2 == 400.0 and c.ba_lambda2 == 400.0
    assert c.tri_str_thresh == np.float32(0.0064) and c.tri_check_str_chi2 == 1 and c.ba_first_as_prior == 1
    # frame::sigma2_inv (init_config.hpp:60-79), float arithmetic
    sf, ref = np.float32(1.0), [np.float32(1.0)]
    for _ in range(7):
        sf = np.float32(sf * np.float32(1.2))
        ref.append(np.float32(1.0) / np.float32(sf * sf))
    assert np.array_equal(p.sigma2_inv, np.array(ref, np.float32))


def test_no_gpu_calls_fail_loudly(lib):
    """Without a device every compute path must return an error, never a CPU result."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = lib.gl_ctx_create(0, None, C.byref(h))
    assert rc != 0 and lib.gl_last_error_string() != b""
    assert lib.gl_device_count() == 0


def test_gmm_file_roundtrip_host(lib, tmp_path):
    from gmmloc_amd import api
    d = np.load(os.path.join(GOLDEN, "map_v1.npz"))
    mean, cov = d["mean"], d["cov"]
    sym = 0.5 * (cov.reshape(-1, 3, 3) + cov.reshape(-1, 3, 3).transpose(0, 2, 1))
    flags = (np.arange(mean.shape[0]) % 4).astype(np.uint8)
    p = tmp_path / "rt.gmm"
    api.write_gmm_file(p, mean, sym.reshape(-1, 9), flags)
    m2, c2 = api.read_gmm_file(p)
    assert np.array_equal(m2, mean) and np.array_equal(c2, sym.reshape(-1, 9))
    assert os.path.getsize(p) == 105 * mean.shape[0] + 2  # 105 B / component


def test_gmm_file_errors(lib, tmp_path):
    from gmmloc_amd import api
    with pytest.raises(api.GLError, match="Could not open"):
        api.read_gmm_file(tmp_path / "nope.gmm")
    (tmp_path / "empty.gmm").write_bytes(b"\x00")
    with pytest.raises(api.GLError, match="empty"):
        api.read_gmm_file(tmp_path / "empty.gmm")
    (tmp_path / "trunc.gmm").write_bytes(b"\x01\x69\x08\x01")
    with pytest.raises(api.GLError):
        api.read_gmm_file(tmp_path / "trunc.gmm")
    # a component with 2 mean values (reference: CHECK_EQ(mean_size, 3) aborts)
    msg = b"\x1a\x10" + np.zeros(2).tobytes() + b"\x22\x48" + np.zeros(9).tobytes()
    (tmp_path / "bad.gmm").write_bytes(b"\x01" + bytes([len(msg)]) + msg)
    with pytest.raises(api.GLError, match="mean_size"):
        api.read_gmm_file(tmp_path / "bad.gmm")
    # unpacked doubles (wire type 1) are accepted like protobuf does
    msg = b"".join(b"\x19" + np.float64(v).tobytes() for v in (1.0, 2.0, 3.0)) + b"\x22\x48" + np.eye(3).tobytes()
    (tmp_path / "unpacked.gmm").write_bytes(b"\x01" + bytes([len(msg)]) + msg)
    m, c = api.read_gmm_file(tmp_path / "unpacked.gmm")
    assert np.array_equal(m, [[1.0, 2.0, 3.0]]) and np.array_equal(c.reshape(3, 3), np.eye(3))
    # lengths near 2^64: `pos + len` wraps, so the reader compares `len > end - pos`.  Each file is read in a child process
    # under a time limit, so a reader that walks out of the buffer or never ends is a failed test, not a crashed or hung suite.
    good = b"\x1a\x18" + np.arange(3.0).tobytes() + b"\x22\x48" + np.eye(3).tobytes()
    huge = lambda n: _varint((1 << 64) - n)
    pad8 = b"\x08\x01" * 4  # eight bytes of field 1 in front, so that pos >= 8
    bad = {
        "size_2p64m1": b"\x01" + huge(1) + good,                                      # a message size of 2^64 - 1
        "packed_2p64m8": _msgs([pad8 + b"\x1a" + huge(8) + np.arange(3.0).tobytes()]),  # packed field 3, len = 2^64 - 8
        "unknown_back_to_tag": _msgs([pad8 + b"\x2a" + huge(11) + b"\x00" * 16]),      # field 5: tag (1) + len (10) bytes back
        "count_over_file": b"\x05" + _msgs([good])[1:],                               # five announced, one present
        "varint_10_continued": b"\xff" * 10 + good,                                   # continuation bit on the tenth byte
    }
    assert len(huge(11)) == 10
    (tmp_path / "good.gmm").write_bytes(_msgs([good]))
    assert _read_in_child(tmp_path / "good.gmm") == "rc=0 K=1"
    for name, data in bad.items():
        (tmp_path / (name + ".gmm")).write_bytes(data)
        assert _read_in_child(tmp_path / (name + ".gmm")) == "rc=-3 K=-1", name  # GL_ERR_FORMAT


def _varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([(v & 0x7F) | 0x80])
        v >>= 7
    return out + bytes([v])


def _msgs(msgs):
    return _varint(len(msgs)) + b"".join(_varint(len(m)) + m for m in msgs)


def _read_in_child(path):
    """gl_gmm_file_read on `path` in a fresh interpreter -> 'rc=<code> K=<count>'; a crash or a hang fails here"""
    import subprocess
    import sys
    from gmmloc_amd import _lib
    code = ("import ctypes as C, sys\nlib = C.CDLL(sys.argv[1])\nK = C.c_int32(-1)\n"  # the library alone: a light child
            "rc = lib.gl_gmm_file_read(sys.argv[2].encode(), None, None, 0, C.byref(K))\nprint('rc=%d K=%d' % (rc, K.value))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH, str(path)], cwd=ROOT, capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, "the reader's process ended with %d: %s" % (r.returncode, r.stderr[-400:])
    return r.stdout.strip()


@pytest.mark.parametrize("name", ["v1", "v2"])
def test_reader_on_the_shipped_maps(lib, name):
    """The C++ reader on the reference's own .gmm files (tests/golden/v{1,2}.gmm, byte-for-byte copies made by
    tools/make_map_fixtures.py) == the independently decoded fixture."""
    from gmmloc_amd import api
    m, c = api.read_gmm_file(os.path.join(GOLDEN, name + ".gmm"))
    d = np.load(os.path.join(GOLDEN, "map_%s.npz" % name))
    assert np.array_equal(m, d["mean"]) and np.array_equal(c, d["cov"])
    assert m.shape[0] == {"v1": 3299, "v2": 5096}[name]


def test_cpp_adapter_compiles_and_reports_errors(lib, tmp_path):
    """The C++ host mirror is plain C++17 over the C-ABI: it builds with g++ (no HIP headers), and without a model
    file loadGMMModel returns false like the reference's loader instead of throwing or crashing."""
    exe = cpp_driver.build("adapter_check", tmp_path)
    r = cpp_driver.run(exe, tmp_path / "missing.gmm", tmp_path / "f.bin", tmp_path / "o.bin", timeout=120)
    assert r.returncode == 1 and "loadGMMModel" in r.stderr
