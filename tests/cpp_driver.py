"""The g++-built drivers of tests/cpp/: one command line to build them, one environment to start them.  They are plain C++17 over
include/gmmloc_hip/gmm_adapter.hpp and the in-tree library (no HIP headers).

Test infrastructure; nothing in the product imports it."""
import os
import subprocess

from tests.conftest import ROOT


def _libdir():
    from gmmloc_amd import _lib
    return os.path.dirname(_lib.LIB_PATH)


def build(name, out_dir):
    """tests/cpp/<name>.cpp -> the executable <out_dir>/<name>"""
    exe = os.path.join(str(out_dir), name)
    libdir = _libdir()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
           "-L" + libdir, "-lgmmloc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, *args, timeout=300):
    """the driver on its arguments -> the completed process, output captured as text; the caller asserts the return code"""
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = _libdir() + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
