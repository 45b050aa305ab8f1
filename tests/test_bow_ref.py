"""The vocabulary reader and the restatement of the DBoW2 transform, on the CPU: tests/bow_ref.py against the declared outputs of
tests/bow_cases.py, gl_voc_file_read against the restatement's reader on files written by gmmloc_amd.synth, and every malformed file
gmmloc_hip.h lists -> GL_ERR_FORMAT (each read in a child process under a time limit, like test_host_cabi.test_gmm_file_errors)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gmmloc_amd import synth
from tests import bow_cases as BC
from tests import bow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("parent", "desc", "weight", "is_leaf")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(BC.CASES))
def test_restatement_gives_the_declared_outputs(name):
    c = BC.CASES[name]
    e = c["expect"]
    word, node, weight, fv = R.transform(R.Tree(c["voc"]), c["desc"], c["oct"], c["levelsup"])
    assert word.tolist() == e["word_id"].tolist()
    assert node.tolist() == e["node"].tolist()
    assert same_bits(weight, e["weight"]), (weight, e["weight"])
    assert [(n, list(f)) for n, f in fv] == e["fv"]


@pytest.mark.parametrize("v", range(4))
def test_every_bit_changes_a_winner(v):
    """the construction of the every_bit_counts cases: feature i of vocabulary v tests bit b = 64 v + i - the winner is the second child
    of its pair, exactly one bit behind it stands the first, that bit is b, and a distance that leaves bit b out elects the first"""
    c = BC.CASES["every_bit_counts_%d" % v]
    children = c["voc"]["desc"]
    for i, f in enumerate(c["desc"]):
        b = 64 * v + i
        diff = np.unpackbits(children ^ f, axis=1, bitorder="little")  # (128, 256): bit p of the xor with child c
        d = diff.sum(1)
        assert int(np.argmin(d)) == 2 * i + 1 and d[2 * i + 1] == 0 and d[2 * i] == 1 and np.nonzero(diff[2 * i])[0].tolist() == [b]
        assert np.sort(d)[2] >= 7
        masked = d - diff[:, b]
        assert int(np.argmin(masked)) == 2 * i, b  # (argmin: the first of the smallest, as `d < best_d`)
        assert c["expect"]["word_id"][i] == 2 * i + 1


def test_negative_levelsup_is_refused():
    c = BC.CASES["levelsup_0"]
    with pytest.raises(ValueError):
        R.transform(R.Tree(c["voc"]), c["desc"], None, -1)


@pytest.fixture(scope="module")
def lib():
    from gmmloc_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("shape", [(2, 1, 0.0), (3, 4, 0.2), (10, 3, 0.1), (1, 5, 0.0)], ids=lambda s: "k%d_L%d" % s[:2])
def test_reader_against_the_restatement(lib, tmp_path, shape):
    from gmmloc_amd import bow
    k, L, early = shape
    v = synth.synth_vocabulary(k, L, seed=7 + k, early_leaf_frac=early)
    v["weight"][:3] = [np.float32("nan"), np.float32(-0.0), BC.F32_DENORM_MIN][:min(3, len(v["weight"]))]
    p = tmp_path / "voc.bin"
    synth.write_vocabulary_file(p, v, scoring=1, weighting=3)
    assert os.path.getsize(p) == 24 + 41 * len(v["parent"])
    got, ref = bow.read_vocabulary_file(p), R.read_file(p)
    for key in KEYS:
        assert same_bits(got[key], ref[key]), key
        assert same_bits(got[key], v[key]), key
    assert (got["k"], got["L"]) == (ref["k"], ref["L"]) == (k, L)


def test_reader_counts_alone_and_capacity(lib, tmp_path):
    import ctypes as C
    v = synth.synth_vocabulary(3, 2, seed=1)
    p = tmp_path / "voc.bin"
    synth.write_vocabulary_file(p, v)
    n, kl = C.c_int(0), (C.c_int * 2)()
    assert lib.gl_voc_file_read(str(p).encode(), None, None, None, None, 0, C.byref(n), kl) == 0
    assert (n.value, kl[0], kl[1]) == (13, 3, 2)
    parent = np.full(12, -9, np.int32)
    assert lib.gl_voc_file_read(str(p).encode(), parent.ctypes.data, None, None, None, 11, C.byref(n), kl) == -1  # GL_ERR_ARG: cap < 12
    assert (parent == -9).all()
    assert lib.gl_voc_file_read(str(p).encode(), parent.ctypes.data, None, None, None, 12, C.byref(n), kl) == 0
    assert parent.tolist() == v["parent"].tolist()
    assert lib.gl_voc_file_read(str(tmp_path / "none.bin").encode(), None, None, None, None, 0, C.byref(n), kl) == -2  # GL_ERR_IO


def _read_in_child(path):
    """gl_voc_file_read on `path` in a fresh interpreter -> 'rc=<code> n=<nodes>'; a crash or a hang fails here"""
    from gmmloc_amd import _lib
    code = ("import ctypes as C, sys\nlib = C.CDLL(sys.argv[1])\nn = C.c_int32(-1)\n"  # the library alone: a light child
            "rc = lib.gl_voc_file_read(sys.argv[2].encode(), None, None, None, None, 0, C.byref(n), None)\nprint('rc=%d n=%d' % (rc, n.value))\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH, str(path)], cwd=ROOT, capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, "the reader's process ended with %d: %s" % (r.returncode, r.stderr[-400:])
    return r.stdout.strip()


def _malformed(tmp_path):
    """name -> path of every kind of file the header declares as refused; 'good' is the file they are all made from"""
    good = synth.synth_vocabulary(2, 2, seed=3, interleave=False)  # nodes 1 2 | 3 4 (of 1) 5 6 (of 2)
    assert good["parent"].tolist() == [0, 0, 1, 1, 2, 2] and good["is_leaf"].tolist() == [0, 0, 1, 1, 1, 1]

    def write(name, **kw):
        v = {key: np.array(val) for key, val in good.items()}
        hdr = {}
        for key, val in kw.items():
            if key in ("nb_nodes", "size_node"):
                hdr[key] = val
            else:
                v[key][val[0]] = val[1]
        p = tmp_path / (name + ".bin")
        synth.write_vocabulary_file(p, v, **hdr)
        return p

    files = {"good": write("good")}
    files["size_node_40"] = write("size_node_40", size_node=40)
    files["size_node_42"] = write("size_node_42", size_node=42)
    files["parent_negative"] = write("parent_negative", parent=(3, -1))
    files["parent_is_itself"] = write("parent_is_itself", parent=(3, 4))        # node 4 names node 4
    files["parent_is_later"] = write("parent_is_later", parent=(2, 6))          # node 3 names node 6: a cycle-free walk never reaches it
    files["parent_far_outside"] = write("parent_far_outside", parent=(5, 2 ** 31 - 1))
    files["leaf_gains_a_child"] = write("leaf_gains_a_child", parent=(5, 3))    # node 6 names the leaf 3
    files["inner_node_without_child"] = write("inner_node_without_child", is_leaf=(5, 0))
    files["inner_node_lost_its_children"] = write("inner_node_lost_its_children", is_leaf=(0, 1))  # node 1 flagged leaf, 3 and 4 name it
    files["nb_nodes_0"] = write("nb_nodes_0", nb_nodes=0)
    files["nb_nodes_1"] = write("nb_nodes_1", nb_nodes=1)
    files["header_says_more"] = write("header_says_more", nb_nodes=8)            # shorter than the header says
    files["header_says_fewer"] = write("header_says_fewer", nb_nodes=6)          # longer
    files["header_says_2p32m1"] = write("header_says_2p32m1", nb_nodes=2 ** 32 - 1)
    data = files["good"].read_bytes()
    for name, cut in (("cut_in_header", data[:20]), ("cut_in_record", data[:-1]), ("one_byte_more", data + b"\x00"), ("header_only", data[:24]),
                      ("empty", b"")):
        files[name] = tmp_path / (name + ".bin")
        files[name].write_bytes(cut)
    only_root = tmp_path / "only_root.bin"
    only_root.write_bytes(np.array([1, 41], "<u4").tobytes() + np.array([10, 6, 0, 0], "<i4").tobytes())
    files["only_root"] = only_root
    return files


def test_malformed_files_are_format_errors(lib, tmp_path):
    files = _malformed(tmp_path)
    assert _read_in_child(files.pop("good")) == "rc=0 n=7"
    for name, p in files.items():
        assert _read_in_child(p) == "rc=-3 n=-1", name  # GL_ERR_FORMAT, nothing reported
        with pytest.raises(R.FormatError):
            R.read_file(p)
