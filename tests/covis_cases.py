"""Hand-built cases for gl_covis_update, gl_covis_remove, gl_covis_best, gl_fuse_targets and gl_fuse_candidates, with DECLARED outputs:
one case on each side of every decision, every output array written out by hand.  tests/test_covis_ref.py holds the object model and
the numpy statement of tests/covis_ref.py to them, tests/test_gpu_covis_cases.py the device.  Test infrastructure.

A graph is written {row: ([(key-frame, weight), ...], cov_nord)}: the row in the declared order and the length of its ordered prefix;
rows not named are empty.  `best` is {row: best_cov}, -1 elsewhere.  graph() makes the arrays, filled with covis_ref.SENTINEL beyond
each row's cov_n.  A map is written as `shared` {(key-frames, ...): n}: n points, each observed by every key-frame of the tuple (a
feature slot of each, taken in order), so the counter of key-frame a names b with the n of every tuple that holds both."""
import numpy as np

from tests.covis_ref import COVIS_BAD_ROW, EMPTY_LIST, KEPT, LIST_TRUNCATED, SENTINEL, TRUNCATED, W_TRUNCATED

NKF, NFK = 7, 64


def graph(nkf, Wcap, rows, best=None):
    g = dict(cov_kf=np.full((nkf, Wcap), SENTINEL, np.int32), cov_w=np.full((nkf, Wcap), SENTINEL, np.int32), cov_n=np.zeros(nkf, np.int32),
             cov_nord=np.zeros(nkf, np.int32), best_cov=np.full(nkf, -1, np.int32))
    for k, (pairs, nord) in rows.items():
        n = len(pairs)
        g["cov_kf"][k, :n] = [a for a, _ in pairs]
        g["cov_w"][k, :n] = [w for _, w in pairs]
        g["cov_n"][k], g["cov_nord"][k] = n, nord
    for k, b in (best or {}).items():
        g["best_cov"][k] = b
    return g


def shared_map(shared, invalid_kf=(), invalid_shared=None, nkf=NKF, nfk=NFK):
    """-> the map dict of covis_ref; invalid_shared: the same notation, points with mp_valid = 0 (held and observing, never counted)"""
    kf_mp = -np.ones((nkf, nfk), np.int32)
    used = [0] * nkf
    ptr, okf, valid = [0], [], []
    for table, ok in ((shared, 1), (invalid_shared or {}, 0)):
        for kfs, n in table.items():
            for _ in range(n):
                p = len(valid)
                for k in kfs:
                    kf_mp[k, used[k]] = p
                    used[k] += 1
                    okf.append(k)
                ptr.append(len(okf))
                valid.append(ok)
    kfv = np.ones(nkf, np.uint8)
    kfv[list(invalid_kf)] = 0
    return dict(kf_mp=kf_mp, mp_valid=np.array(valid, np.uint8), obs_ptr=np.array(ptr, np.int32), obs_kf=np.array(okf, np.int32), kf_valid=kfv)


# ================================================================================================ gl_covis_update (key-frame 0)
# name -> dict(shared[, invalid_kf, invalid_shared], rows0, [best0,] Wcap, Ccap, out = dict(rows, conn, n_conn, result))
# result = {widest row, status, other rows changed, 0}; conn: the entries conn_kf / conn_w hold (0 behind them)
NB_2_OF_5 = ([(2, 30), (0, 16), (3, 9), (4, 8), (5, 7)], 2)
UPDATE = {
    # 15 is listed and told, 14 is in the weights only: the prefix ends in front of it
    "14_against_15": dict(
        shared={(0, 1): 15, (0, 2): 14, (0, 3): 20}, rows0={}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(3, 20), (1, 15), (2, 14)], 2), 1: ([(0, 15)], 1), 3: ([(0, 20)], 1)}, conn=[(3, 20), (1, 15)], n_conn=2,
                 result=[3, 0, 2, 0])),
    "conn_cap_below": dict(
        shared={(0, 1): 15, (0, 2): 14, (0, 3): 20}, rows0={}, Wcap=6, Ccap=1,
        out=dict(rows={0: ([(3, 20), (1, 15), (2, 14)], 2), 1: ([(0, 15)], 1), 3: ([(0, 20)], 1)}, conn=[(3, 20)], n_conn=2,
                 result=[3, TRUNCATED, 2, 0])),
    # none reaches 15: the single largest is listed and told
    "none_reaches_15": dict(
        shared={(0, 1): 9, (0, 2): 12}, rows0={}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(2, 12), (1, 9)], 1), 2: ([(0, 12)], 1)}, conn=[(2, 12)], n_conn=1, result=[2, 0, 1, 0])),
    # ... and a tie for it goes to the lowest row
    "tie_for_the_largest": dict(
        shared={(0, 4): 9, (0, 2): 9, (0, 1): 3}, rows0={}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(2, 9), (4, 9), (1, 3)], 1), 2: ([(0, 9)], 1)}, conn=[(2, 9)], n_conn=1, result=[3, 0, 1, 0])),
    # a tie at 15 and above: both listed, the lower row first
    "tie_of_listed": dict(
        shared={(0, 5): 17, (0, 3): 17}, rows0={}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(3, 17), (5, 17)], 2), 3: ([(0, 17)], 1), 5: ([(0, 17)], 1)}, conn=[(3, 17), (5, 17)], n_conn=2, result=[2, 0, 2, 0])),
    # addConnection on a neighbour whose ordered list is 2 of its entries: absent -> inserted in order, the list becomes the WHOLE row
    "add_absent": dict(
        shared={(0, 1): 16}, rows0={1: ([(2, 30), (3, 20), (4, 9), (5, 8)], 2)}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 16)], 1), 1: ([(2, 30), (3, 20), (0, 16), (4, 9), (5, 8)], 5)}, conn=[(1, 16)], n_conn=1, result=[5, 0, 1, 0])),
    # present with another weight -> changed and moved, the list becomes the whole row, entries below 15 in it
    "add_changed": dict(
        shared={(0, 1): 16}, rows0={1: ([(0, 40), (2, 30), (3, 20), (4, 9), (5, 8)], 2)}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 16)], 1), 1: ([(2, 30), (3, 20), (0, 16), (4, 9), (5, 8)], 5)}, conn=[(1, 16)], n_conn=1, result=[5, 0, 1, 0])),
    # present with the same weight -> nothing: the prefix of 2 out of 5 stays
    "add_same": dict(
        shared={(0, 1): 16}, rows0={1: NB_2_OF_5}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 16)], 1), 1: NB_2_OF_5}, conn=[(1, 16)], n_conn=1, result=[5, 0, 0, 0])),
    # the own row is REPLACED by the counter (:312): what it named before is gone, whatever names IT stays
    "own_row_replaced": dict(
        shared={(0, 1): 16}, rows0={0: ([(5, 33), (1, 2)], 2), 5: ([(0, 33)], 1)}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 16)], 1), 1: ([(0, 16)], 1), 5: ([(0, 33)], 1)}, conn=[(1, 16)], n_conn=1, result=[1, 0, 1, 0])),
    # an empty counter: nothing changes, the old row included
    "empty_counter": dict(
        shared={(1, 2): 20}, rows0={0: ([(1, 20)], 1)}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 20)], 1)}, conn=[], n_conn=0, result=[0, KEPT, 0, 0])),
    # an invalid observer is counted and gains the entry; an invalid POINT is not counted
    "invalid_observer": dict(
        shared={(0, 1): 15}, invalid_kf=(1,), invalid_shared={(0, 2): 20}, rows0={}, Wcap=6, Ccap=4,
        out=dict(rows={0: ([(1, 15)], 1), 1: ([(0, 15)], 1)}, conn=[(1, 15)], n_conn=1, result=[1, 0, 1, 0])),
    # a neighbour's row would need a third entry: refused, the graph as it was, the width in result[0]
    "w_truncated": dict(
        shared={(0, 1): 16}, rows0={1: ([(2, 30), (3, 20)], 2)}, Wcap=2, Ccap=4,
        out=dict(rows={1: ([(2, 30), (3, 20)], 2)}, conn=[(1, 16)], n_conn=1, result=[3, W_TRUNCATED, 0, 0])),
    # ... and at the width it needs
    "w_at_the_need": dict(
        shared={(0, 1): 16}, rows0={1: ([(2, 30), (3, 20)], 2)}, Wcap=3, Ccap=4,
        out=dict(rows={0: ([(1, 16)], 1), 1: ([(2, 30), (3, 20), (0, 16)], 3)}, conn=[(1, 16)], n_conn=1, result=[3, 0, 1, 0])),
}

# ================================================================================================ gl_covis_remove
# name -> dict(rows0, best0, list, [n_cull,] kf_first, out = dict(rows, best, result)); result = {removed, status, erased, malformed}
TRIANGLE = {1: ([(2, 20), (3, 16)], 2), 2: ([(1, 20), (3, 18)], 1), 3: ([(2, 18), (1, 16)], 1)}
ONE_SIDED = {1: ([(2, 20)], 1), 2: ([(1, 20)], 1), 3: ([(1, 17)], 1)}  # 3 names 1, 1 does not name 3
REMOVE = {
    # the row 1 names loses its entry; the row that names 1 one-sidedly keeps a dangling one
    "dangling": dict(rows0=ONE_SIDED, best0={}, list=[1], kf_first=0,
                     out=dict(rows={3: ([(1, 17)], 1)}, best={1: 2}, result=[1, 0, 1, 0])),
    # two listed rows that name each other: the first removal rewrites the second's row before it is removed
    "pair_1_then_2": dict(rows0=TRIANGLE, best0={}, list=[1, 2], kf_first=0,
                          out=dict(rows={}, best={1: 2, 2: 3}, result=[2, 0, 3, 0])),
    "pair_2_then_1": dict(rows0=TRIANGLE, best0={}, list=[2, 1], kf_first=0,
                          out=dict(rows={}, best={2: 1, 1: 3}, result=[2, 0, 3, 0])),
    # one removal: the rows that lose an entry list their WHOLE row afterwards (1 of 2 -> 1 of 1)
    "prefix_becomes_whole": dict(rows0={1: ([(2, 20), (3, 16)], 2), 2: ([(4, 30), (1, 20), (3, 18)], 1), 3: ([(2, 18), (1, 16)], 1)}, best0={}, list=[1],
                                 kf_first=0, out=dict(rows={2: ([(4, 30), (3, 18)], 2), 3: ([(2, 18)], 1)}, best={1: 2}, result=[1, 0, 2, 0])),
    "kf_first_in_the_list": dict(rows0=ONE_SIDED, best0={}, list=[1], kf_first=1,
                                 out=dict(rows=ONE_SIDED, best={}, result=[0, 0, 0, 0])),
    # listed twice: the second occurrence meets an empty list - best_cov stays what the first made it
    "listed_twice": dict(rows0=ONE_SIDED, best0={}, list=[1, 1], kf_first=0,
                         out=dict(rows={3: ([(1, 17)], 1)}, best={1: 2}, result=[2, EMPTY_LIST, 1, 0])),
    "empty_list": dict(rows0=ONE_SIDED, best0={4: 6}, list=[4], kf_first=0,
                       out=dict(rows=ONE_SIDED, best={4: 6}, result=[1, EMPTY_LIST, 0, 0])),
    "rows_outside_the_table": dict(rows0=ONE_SIDED, best0={}, list=[NKF, -1, 1], kf_first=0,
                                   out=dict(rows={3: ([(1, 17)], 1)}, best={1: 2}, result=[1, COVIS_BAD_ROW, 1, 2])),
    "count_on_the_device": dict(rows0=TRIANGLE, best0={}, list=[1, 2], n_cull=1, kf_first=0,
                                out=dict(rows={2: ([(3, 18)], 1), 3: ([(2, 18)], 1)}, best={1: 2}, result=[1, 0, 2, 0])),
}

# ================================================================================================ gl_covis_best
# on one graph: (rows, N, Ccap) -> per row the entries, n_conn; status
BEST_ROWS = {1: ([(2, 30), (3, 20), (4, 9), (5, 8)], 3), 2: ([(1, 30)], 1)}
BEST = {
    "below": dict(kf=[1, 2, 6], N=2, Ccap=4, out=dict(conn=[[(2, 30), (3, 20)], [(1, 30)], []], n_conn=[2, 1, 0], result=[0, 0, 0, 0])),
    "at": dict(kf=[1], N=3, Ccap=4, out=dict(conn=[[(2, 30), (3, 20), (4, 9)]], n_conn=[3], result=[0, 0, 0, 0])),
    "above": dict(kf=[1], N=4, Ccap=4, out=dict(conn=[[(2, 30), (3, 20), (4, 9)]], n_conn=[3], result=[0, 0, 0, 0])),
    "all": dict(kf=[1], N=0, Ccap=4, out=dict(conn=[[(2, 30), (3, 20), (4, 9)]], n_conn=[3], result=[0, 0, 0, 0])),
    "cap_below": dict(kf=[1, NKF], N=0, Ccap=2, out=dict(conn=[[(2, 30), (3, 20)], []], n_conn=[3, 0], result=[0, TRUNCATED | COVIS_BAD_ROW, 0, 1])),
}

# ================================================================================================ gl_fuse_targets (key-frame 0)
# name -> dict(nkf, rows, [invalid_kf,] nn, nn2, Tcap, out = dict(tgt, n_tgt, result)); a row [(k, w), ...] written as keys only below
def _row(keys, nord=None, w0=60):
    return ([(k, w0 - i) for i, k in enumerate(keys)], len(keys) if nord is None else nord)


TARGETS = {
    # eleven neighbours: the tenth is a target, the eleventh is not
    "tenth_against_eleventh": dict(nkf=13, rows={0: _row(range(1, 12))}, nn=10, nn2=5, Tcap=60,
                                   out=dict(tgt=list(range(1, 11)), n_tgt=10, result=[10, 0, 0, 0])),
    # six second neighbours: the fifth is a target, the sixth is not
    "fifth_against_sixth": dict(nkf=9, rows={0: _row([1]), 1: _row([2, 3, 4, 5, 6, 7])}, nn=10, nn2=5, Tcap=60,
                                out=dict(tgt=[1, 2, 3, 4, 5, 6], n_tgt=6, result=[6, 0, 0, 0])),
    # the ordered PREFIX is what is read, not the row: 3 of 6
    "prefix_of_the_row": dict(nkf=9, rows={0: _row([1]), 1: _row([2, 3, 4, 5, 6, 7], nord=3)}, nn=10, nn2=5, Tcap=60,
                              out=dict(tgt=[1, 2, 3, 4], n_tgt=4, result=[4, 0, 0, 0])),
    # an invalid kf1 is skipped WITH its second neighbours: 3 would qualify
    "invalid_kf1": dict(nkf=7, rows={0: _row([1, 2]), 1: _row([3]), 2: _row([4])}, invalid_kf=(1,), nn=10, nn2=5, Tcap=60,
                        out=dict(tgt=[2, 4], n_tgt=2, result=[2, 0, 0, 0])),
    # kf1 = 2 entered earlier as the second neighbour of 1: skipped with ITS second neighbours, 5 stays out
    "kf1_entered_earlier": dict(nkf=7, rows={0: _row([1, 2]), 1: _row([2, 3]), 2: _row([5])}, nn=10, nn2=5, Tcap=60,
                                out=dict(tgt=[1, 2, 3], n_tgt=3, result=[3, 0, 0, 0])),
    # kf2 == the key-frame itself, an invalid kf2, a kf2 that is already a target, an entry outside the table
    "kf2_skipped": dict(nkf=7, rows={0: _row([1, 4]), 1: _row([0, 6, 2, 9]), 4: _row([1, 3])}, invalid_kf=(6,), nn=10, nn2=5, Tcap=60,
                        out=dict(tgt=[1, 2, 4, 3], n_tgt=4, result=[4, COVIS_BAD_ROW, 0, 1])),
    "tcap_at": dict(nkf=9, rows={0: _row([1]), 1: _row([2, 3, 4, 5, 6, 7])}, nn=10, nn2=5, Tcap=6,
                    out=dict(tgt=[1, 2, 3, 4, 5, 6], n_tgt=6, result=[6, 0, 0, 0])),
    "tcap_below": dict(nkf=9, rows={0: _row([1]), 1: _row([2, 3, 4, 5, 6, 7])}, nn=10, nn2=5, Tcap=5,
                       out=dict(tgt=[1, 2, 3, 4, 5], n_tgt=6, result=[6, LIST_TRUNCATED, 0, 0])),
    "no_neighbours": dict(nkf=3, rows={}, nn=10, nn2=5, Tcap=4, out=dict(tgt=[], n_tgt=0, result=[0, 0, 0, 0])),
}
# (kf1_entered_earlier: 1 enters, then 2 and 3 as its second neighbours; at kf1 = 2 the `continue` of :162-164 drops 5)

# ================================================================================================ gl_fuse_candidates
# four key-frames of four slots, six points (3 invalid, 5 held by nobody); name -> dict(tgt, n_tgt, kf_idx, cand_cap, out)
CAND_KF_MP = [[-1, -1, -1, -1], [0, 1, -1, 2], [1, 3, 4, -1], [4, 4, 6, -7]]
CAND_MP_VALID = [1, 1, 1, 0, 1, 1]


def cand_map():
    ptr = np.zeros(len(CAND_MP_VALID) + 1, np.int32)
    return dict(kf_mp=np.array(CAND_KF_MP, np.int32), mp_valid=np.array(CAND_MP_VALID, np.uint8), obs_ptr=ptr, obs_kf=np.zeros(0, np.int32),
                kf_valid=np.ones(4, np.uint8))


CANDIDATES = {
    # point 1 is held by both targets: appended at its first occurrence; the null slot and the invalid point 3 are skipped
    "first_occurrence": dict(tgt=[1, 2], n_tgt=2, kf_idx=7, cand_cap=8, out=dict(cand=[0, 1, 2, 4], n_cand=4, result=[4, 0, 0, 0])),
    "other_order": dict(tgt=[2, 1], n_tgt=2, kf_idx=7, cand_cap=8, out=dict(cand=[1, 4, 0, 2], n_cand=4, result=[4, 0, 0, 0])),
    # a point twice in one key-frame, slots outside the point table
    "twice_in_a_row": dict(tgt=[3], n_tgt=1, kf_idx=7, cand_cap=8, out=dict(cand=[4], n_cand=1, result=[1, 0, 0, 0])),
    # fuse_tgt_kf_ starts at 0: for key-frame 0 every point looks stamped
    "kf_idx_0": dict(tgt=[1, 2], n_tgt=2, kf_idx=0, cand_cap=8, out=dict(cand=[], n_cand=0, result=[0, 0, 0, 0])),
    "cap_at": dict(tgt=[1, 2], n_tgt=2, kf_idx=7, cand_cap=4, out=dict(cand=[0, 1, 2, 4], n_cand=4, result=[4, 0, 0, 0])),
    "cap_below": dict(tgt=[1, 2], n_tgt=2, kf_idx=7, cand_cap=3, out=dict(cand=[0, 1, 2], n_cand=4, result=[4, LIST_TRUNCATED, 0, 0])),
    "count_on_the_device": dict(tgt=[1, 2], n_tgt=1, kf_idx=7, cand_cap=8, out=dict(cand=[0, 1, 2], n_cand=3, result=[3, 0, 0, 0])),
    "target_outside_the_table": dict(tgt=[1, 9, 2], n_tgt=3, kf_idx=7, cand_cap=8, out=dict(cand=[0, 1, 2, 4], n_cand=4, result=[4, COVIS_BAD_ROW, 0, 1])),
    "no_targets": dict(tgt=[1, 2], n_tgt=0, kf_idx=7, cand_cap=8, out=dict(cand=[], n_cand=0, result=[0, 0, 0, 0])),
}


# ================================================================================================ checking a graph against a declaration
def assert_graph(g, g0, rows, best, what=""):
    """g holds exactly the declared rows (cov_n, cov_nord, the entries in front of cov_n) and best_cov; behind the longer of a row's old
    and new length every word is what g0 (the graph on entry) held - the sentinel"""
    nkf, W = g["cov_kf"].shape
    for k in range(nkf):
        pairs, nord = rows.get(k, ([], 0))
        n = len(pairs)
        assert (int(g["cov_n"][k]), int(g["cov_nord"][k])) == (n, nord), (what, k, int(g["cov_n"][k]), int(g["cov_nord"][k]), n, nord)
        got = list(zip(g["cov_kf"][k, :n].tolist(), g["cov_w"][k, :n].tolist()))
        assert got == [tuple(p) for p in pairs], (what, k, got, pairs)
        tail = max(n, int(g0["cov_n"][k]))
        for a in ("cov_kf", "cov_w"):
            assert np.array_equal(g[a][k, tail:], g0[a][k, tail:]), (what, k, a, "written behind the row")
    want = np.full(nkf, -1, np.int32)
    for k, b in best.items():
        want[k] = b
    assert np.array_equal(g["best_cov"], want), (what, g["best_cov"], want)


def assert_list(arr, want, what=""):
    """arr starts with the declared list and is untouched (0) behind it"""
    assert arr[:len(want)].tolist() == list(want) and not arr[len(want):].any(), (what, arr.tolist(), want)


# ================================================================================================ random maps and edit sequences
R_NKF, R_NFK, R_NMP = 40, 32, 600


def random_map(seed):
    """about R_NMP points over R_NKF key-frames of R_NFK slots: a point is seen from a key-frame and, with falling probability, from the
    next three, so that neighbours share from a few to more than 15 points"""
    rng = np.random.default_rng(seed)
    kf_mp = -np.ones((R_NKF, R_NFK), np.int32)
    used = [0] * R_NKF
    ptr, okf = [0], []
    for p in range(R_NMP):
        b = int(rng.integers(R_NKF))
        ks = [b] + [b + d for d, pr in ((1, 0.85), (2, 0.45), (3, 0.2)) if b + d < R_NKF and rng.random() < pr]
        for k in ks:
            if used[k] < R_NFK:
                kf_mp[k, used[k]] = p
                used[k] += 1
                okf.append(k)
        ptr.append(len(okf))
    return dict(kf_mp=kf_mp, mp_valid=np.ones(R_NMP, np.uint8), obs_ptr=np.array(ptr, np.int32), obs_kf=np.array(okf, np.int32),
                kf_valid=np.ones(R_NKF, np.uint8))


def random_steps(seed, n):
    """n edits: ("update", kf) | ("remove", [rows], kf_first) | ("flip", points) - the last changes mp_valid, so that later counters differ
    from the weights stored (addConnection's changed-weight branch) and counts cross 15 in both directions"""
    rng = np.random.default_rng(seed)
    steps = []
    for _ in range(n):
        u = rng.random()
        if u < 0.6:
            steps.append(("update", int(rng.integers(R_NKF))))
        elif u < 0.8:
            steps.append(("flip", rng.integers(0, R_NMP, 25).tolist()))
        else:
            steps.append(("remove", rng.integers(0, R_NKF, int(rng.integers(1, 4))).tolist(), int(rng.integers(0, 3))))
    return steps
