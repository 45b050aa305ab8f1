"""Hand-built vocabularies and descriptors for the DBoW2 transform, every output written out: one case on each side of every decision
of TemplatedVocabulary::transform (TemplatedVocabulary.h:1241-1283, :1150-1218) and of the declared behaviours of gmmloc_hip.h.
tests/test_bow_ref.py holds the restatement (tests/bow_ref.py) to them, tests/test_gpu_bow_cases.py the device.

A case: voc (the dict of bow_ref / synth_vocabulary), desc (NF,32) u8, oct (NF,) i32 or None, levelsup, and `expect`: word_id, node,
weight per feature and fv = [(node id, [features])] in the order of the feature vector.  Node ids are record number + 1; in a flat
vocabulary (the root's children are all leaves) child position c is node c + 1 and word c."""
import numpy as np

F32_DENORM_MIN = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]
NEG_ZERO = np.float32(-0.0)
NAN = np.float32("nan")


def bits(*pos):
    """the 32-byte descriptor with exactly these bits set (bit p = bit p % 8 of byte p // 8)"""
    d = np.zeros(32, np.uint8)
    for p in pos:
        d[p // 8] |= np.uint8(1 << (p % 8))
    return d


def voc(parent, desc, weight=None, is_leaf=None, L=1, k=0):
    parent = np.asarray(parent, np.int32)
    n = len(parent)
    if is_leaf is None:  # a node is a leaf iff nobody names it as parent
        is_leaf = np.array([0 if (i + 1) in set(parent.tolist()) else 1 for i in range(n)], np.uint8)
    weight = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32)
    return dict(parent=parent, desc=np.stack(desc).astype(np.uint8), weight=weight, is_leaf=np.asarray(is_leaf, np.uint8), k=k, L=L)


def flat(n):
    """n leaves under the root, L = 1; child c holds the seven bits 7 c .. 7 c + 6 (n <= 36): disjoint, every pair 14 apart"""
    return voc([0] * n, [bits(*range(7 * c, 7 * c + 7)) for c in range(n)], L=1, k=n)


def near(a, b):
    """three bits of child a and three of child b of flat(): distance 7 to both, 13 to every other child"""
    return bits(*range(7 * a, 7 * a + 3), *range(7 * b, 7 * b + 3))


def case(voc, desc, expect_child=None, levelsup=0, oct=None, **expect):
    desc = np.stack(desc).astype(np.uint8)
    if expect_child is not None:  # flat vocabulary, weight 1, levelsup 0: word = child, node = child + 1, every feature kept
        ch = np.asarray(expect_child, np.int32)
        fv = {}
        for i, c in enumerate(ch.tolist()):
            fv.setdefault(c + 1, []).append(i)
        expect = dict(word_id=ch, node=ch + 1, weight=np.ones(len(ch), np.float32), fv=sorted(fv.items()))
    expect = dict(word_id=np.asarray(expect["word_id"], np.int32), node=np.asarray(expect["node"], np.int32),
                  weight=np.asarray(expect["weight"], np.float32), fv=[(int(n), list(f)) for n, f in expect["fv"]])
    return dict(voc=voc, desc=desc, oct=None if oct is None else np.asarray(oct, np.int32), levelsup=levelsup, expect=expect)


CASES = {}

# ---- ties: the FIRST of two children at equal distance wins (`d < best_d`), wherever the pair sits in the chunks of 16 ----------------
CASES["tie_0_1_of_2"] = case(flat(2), [near(0, 1), near(1, 0)], expect_child=[0, 0])
CASES["tie_8_9_of_10"] = case(flat(10), [near(8, 9), near(9, 8), near(9, 9)], expect_child=[8, 8, 9])
CASES["tie_15_16_of_17"] = case(flat(17), [near(15, 16), near(16, 15), near(16, 16)], expect_child=[15, 15, 16])
CASES["tie_16_17_and_31_32_of_33"] = case(flat(33), [near(16, 17), near(31, 32), near(32, 32), near(0, 32), near(15, 31)],
                                          expect_child=[16, 31, 32, 0, 15])
# a node with one child: it is taken whatever its distance (256 here)
CASES["one_child"] = case(voc([0], [bits()], L=1), [bits(*range(256)), bits()], expect_child=[0, 0])


def _flat255():
    """child c holds the byte c + 1 in front; child 254 is a copy of child 200 (0xC9)"""
    d = [np.array([c + 1] + [0] * 31, np.uint8) for c in range(255)]
    d[254] = d[200].copy()
    return voc([0] * 255, d, L=1, k=255)


# 0xC9: children 200 and 254 at distance 0 -> 200.  0xFF: no child holds it (254's byte is 0xC9); distance 1 to 0x7F (child 126), 0xBF
# (190), 0xDF, 0xEF, 0xF7, 0xFB, 0xFD, 0xFE (253) -> the first, 126.  0xFE: child 253 alone at distance 0, in the last chunk.
CASES["children_255"] = case(_flat255(), [np.array([0xC9] + [0] * 31, np.uint8), np.array([0xFF] + [0] * 31, np.uint8),
                                          np.array([0xFE] + [0] * 31, np.uint8)], expect_child=[200, 126, 253])

# ---- distance arithmetic -----------------------------------------------------------------------------------------------------------------
ONES = bits(*range(256))
CASES["distance_0_and_256"] = case(voc([0, 0], [bits(), ONES], L=1), [bits(), ONES, bits(*range(128)), bits(*range(129))],
                                   expect_child=[0, 1, 0, 1])  # (0, 256), (256, 0), (128, 128) -> first, (129, 127)


# Every one of the 256 bits is counted: for bit b the pair of children L_b = {b + 64, b + 128, b + 192} (mod 256), listed FIRST, and
# W_b = L_b + {b}, and the feature W_b itself: 1 to L_b - the one bit is b -, 0 to W_b -> the second of the pair.  With bit b left
# out of the distance both are at 0 and the first, L_b, wins.  Four flat vocabularies of 128 children, bits 64 v .. 64 v + 63 each (no
# two of a vocabulary's bits agree mod 64, so the pairs are disjoint: every other child is 7 or 8 away); W_b sits at the odd position
# 2 (b - 64 v) + 1, in every lane parity and every chunk of 16.  tests/test_bow_ref.py checks the construction itself.
def bit_pair(b):
    lo = [(b + 64 * q) % 256 for q in (1, 2, 3)]
    return bits(*lo), bits(b, *lo)


for _v in range(4):
    _pairs = [bit_pair(b) for b in range(64 * _v, 64 * _v + 64)]
    CASES["every_bit_counts_%d" % _v] = case(voc([0] * 128, [d for p in _pairs for d in p], L=1, k=128), [p[1] for p in _pairs],
                                            expect_child=[2 * i + 1 for i in range(64)])

# ---- stopped words: weight > 0 is false for 0.0f, -0.0f and NaN; the feature keeps its word and its node ---------------------------------
_W = [np.float32(0.0), NEG_ZERO, NAN, F32_DENORM_MIN, np.float32(1.0)]
_f5 = flat(5)
_f5["weight"] = np.array(_W, np.float32)
CASES["stopped_words"] = case(_f5, [near(c, c) for c in (4, 3, 2, 1, 0, 3)], word_id=[4, 3, 2, 1, 0, 3], node=[5, 4, 3, 2, 1, 4],
                              weight=[_W[4], _W[3], _W[2], _W[1], _W[0], _W[3]], fv=[(4, [1, 5]), (5, [0])])
_f2 = flat(2)
_f2["weight"] = np.array([0.0, NAN], np.float32)
CASES["all_stopped"] = case(_f2, [near(0, 0), near(1, 1), near(0, 1)], word_id=[0, 1, 0], node=[1, 2, 1], weight=[0.0, NAN, 0.0], fv=[])


# ---- levels: a binary tree of depth 3, ids level by level: 1 2 | 3 4 (of 1) 5 6 (of 2) | 7 8 (of 3) 9 10 (of 4) 11 12 (of 5) 13 14 (of 6)
def _deep():
    parent = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    # node n holds the bits of its path: level 1 -> bits 0-9 / 10-19, level 2 -> + 20-29 / 30-39, level 3 -> + 40-49 / 50-59
    d = {}
    for n in range(1, 15):
        p = parent[n - 1]
        lvl = 1 if p == 0 else (2 if p <= 2 else 3)
        second = (n - 1) % 2 if lvl == 1 else (n - 3) % 2 if lvl == 2 else (n - 7) % 2
        own = range(20 * (lvl - 1) + 10 * second, 20 * (lvl - 1) + 10 * second + 10)
        d[n] = (d[p] if p else []) + list(own)
    return voc(parent, [bits(*d[n]) for n in range(1, 15)], weight=np.arange(1, 15, dtype=np.float32), L=3, k=2), d


_DEEP, _PATH = _deep()
_DEEP_DESC = [bits(*_PATH[14]), bits(*_PATH[7]), bits(*_PATH[10]), bits(*_PATH[13]), bits(*_PATH[8])]  # leaves 14 7 10 13 8: words 7 0 3 6 1
_DEEP_W = [14.0, 7.0, 10.0, 13.0, 8.0]
CASES["levelsup_0"] = case(_DEEP, _DEEP_DESC, levelsup=0, word_id=[7, 0, 3, 6, 1], node=[14, 7, 10, 13, 8], weight=_DEEP_W,
                           fv=[(7, [1]), (8, [4]), (10, [2]), (13, [3]), (14, [0])])
CASES["levelsup_1"] = case(_DEEP, _DEEP_DESC, levelsup=1, word_id=[7, 0, 3, 6, 1], node=[6, 3, 4, 6, 3], weight=_DEEP_W,
                           fv=[(3, [1, 4]), (4, [2]), (6, [0, 3])])
CASES["levelsup_L_minus_1"] = case(_DEEP, _DEEP_DESC, levelsup=2, word_id=[7, 0, 3, 6, 1], node=[2, 1, 1, 2, 1], weight=_DEEP_W,
                                   fv=[(1, [1, 2, 4]), (2, [0, 3])])
CASES["levelsup_L"] = case(_DEEP, _DEEP_DESC, levelsup=3, word_id=[7, 0, 3, 6, 1], node=[0] * 5, weight=_DEEP_W, fv=[(0, [0, 1, 2, 3, 4])])
CASES["levelsup_L_plus_3"] = case(_DEEP, _DEEP_DESC, levelsup=6, word_id=[7, 0, 3, 6, 1], node=[0] * 5, weight=_DEEP_W, fv=[(0, [0, 1, 2, 3, 4])])
CASES["L_1_levelsup_4"] = case(flat(3), [near(2, 2), near(0, 0), near(1, 1)], levelsup=4, word_id=[2, 0, 1], node=[0, 0, 0], weight=[1, 1, 1],
                               fv=[(0, [0, 1, 2])])
# a leaf two levels above the level asked for: node 1 is a leaf at level 1, node 2 has the children 3, 4 whose children are 5 .. 8;
# L = 3, levelsup = 0.  DECLARED: the feature that stops at node 1 gets node 1.
_SHALLOW = voc([0, 0, 2, 2, 3, 3, 4, 4], [bits(0), bits(1), bits(1, 2), bits(1, 3), bits(1, 2, 4), bits(1, 2, 5), bits(1, 3, 4), bits(1, 3, 5)],
               weight=[1.5, 9, 9, 9, 2.5, 3.5, 4.5, 5.5], L=3, k=2)
CASES["shallow_leaf"] = case(_SHALLOW, [bits(0), bits(1, 3, 5), bits(0), bits(1, 2, 4)], levelsup=0, word_id=[0, 4, 0, 1], node=[1, 8, 1, 5],
                             weight=[1.5, 5.5, 1.5, 2.5], fv=[(1, [0, 2]), (5, [3]), (8, [1])])
CASES["shallow_leaf_levelsup_1"] = case(_SHALLOW, [bits(0), bits(1, 3, 5), bits(1, 2, 4)], levelsup=1, word_id=[0, 4, 1], node=[1, 4, 3],
                                        weight=[1.5, 5.5, 2.5], fv=[(1, [0]), (3, [2]), (4, [1])])

# ---- node order: ids not monotone in tree position.  Node 1 has the children 3 and 5, node 2 the children 4 and 6 (interleaved in the
# file); the features find 6, 3, 5, 4, 5: the feature vector is ascending by id, not in the order of discovery, nor of the tree -----------
_INTER = voc([0, 0, 1, 2, 1, 2], [bits(0), bits(1), bits(0, 2), bits(1, 2), bits(0, 3), bits(1, 3)], weight=[9, 9, 1, 2, 3, 4], L=2, k=2)
CASES["interleaved_ids"] = case(_INTER, [bits(1, 3), bits(0, 2), bits(0, 3), bits(1, 2), bits(0, 3)], levelsup=0, word_id=[3, 0, 2, 1, 2],
                                node=[6, 3, 5, 4, 5], weight=[4, 1, 3, 2, 3], fv=[(3, [1]), (4, [3]), (5, [2, 4]), (6, [0])])

# ---- the last record of the file is the unique nearest child, at distance 0.  The reference's loader reads one record too many and
# appends a copy of the last record to its parent as a further child and word (the phantom, declared deviation 1): it stands behind the
# last child at the same distance, and only the strict `d < best_d` keeps it out - word 4, not the phantom's word 5.  The last record
# under an inner node: node 14 of _DEEP, feature 0 of levelsup_0 ------------------------------------------------------------------------
CASES["last_record_nearest"] = case(flat(5), [bits(*range(28, 35)), near(4, 4), near(3, 4)], expect_child=[4, 4, 3])

# ---- padding slots (oct < 0) at both ends: no feature, -1 / -1 / 0 -----------------------------------------------------------------------
CASES["padding_both_ends"] = case(flat(3), [near(0, 0), near(2, 2), near(1, 1), near(2, 2), near(0, 0)], oct=[-1, 0, 3, 7, -1],
                                  word_id=[-1, 2, 1, 2, -1], node=[-1, 3, 2, 3, -1], weight=[0, 1, 1, 1, 0], fv=[(2, [2]), (3, [1, 3])])
CASES["padding_everywhere"] = case(flat(3), [near(0, 0), near(2, 2)], oct=[-1, -5], word_id=[-1, -1], node=[-1, -1], weight=[0, 0], fv=[])
