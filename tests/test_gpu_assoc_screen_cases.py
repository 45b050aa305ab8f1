"""GPU: every declared case of tests/assoc_screen_cases.py through GL_ASSOC_SCREENED.  idx and d2 equal GL_ASSOC_EXHAUSTIVE's bit for
bit and the model's (tests/assoc_model.py), and GL_COUNTER_ASSOC_SCREEN_VERIFIED / _FALLBACK equal the integers the host model of
gl_assoc32.hip (tests/assoc_screen_model.py) declares - exactly: at the ladders one fp32 ulp in any intermediate of the screen
changes the count, and the compaction, kOut, split and lane cases change it with any slip in the lists' bookkeeping.  The CPU side
(tests/test_assoc_screen_cases.py) asserts that each case reaches the launch shape and the path through note() it was built for.

The cases marked `brute` (ladders, tails, splits, kOut, lanes) also go through GL_ASSOC_BRUTE with assoc_screen32 = 1 below
assoc_index_min, the other caller of the same launch: same counters, same bits.

The listed-subset caller (list / count_dev: the remainder of the cell index) is not declared here: which points the index leaves
unresolved depends on the grid build_cell_index chooses for the map, which tests/assoc_model.py does not model in full; that route
is left to tests/test_gpu_assoc_screened.py::test_option_routes_index_remainder.
"""
import numpy as np
import pytest

from gmmloc_amd import api
from tests import assoc_screen_cases as sc

pytestmark = pytest.mark.gpu

VER, FB = api.COUNTER_ASSOC_SCREEN_VERIFIED, api.COUNTER_ASSOC_SCREEN_FALLBACK


def counted(torch, ctx, g, pts, mode):
    ctx.counter_read(VER)
    ctx.counter_read(FB)
    idx, d2 = g.associate3d(pts, mode)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), (ctx.counter_read(VER), ctx.counter_read(FB))


@pytest.mark.parametrize("name", sc.names())
def test_declared_counters(gpu, opt, name):
    torch, ctx = gpu
    c = sc.CASES[name]
    g = api.GMM(ctx, c.mean, c.cov.reshape(-1, 9))
    pts = torch.from_numpy(c.full_points()).cuda()
    assert len(pts) == c.N
    ref = c.reference()
    which = np.arange(c.N) % len(c.pts)
    want_idx, want_d2 = ref["idx"][which], ref["d2"][which]
    ie, de, none = counted(torch, ctx, g, pts, api.ASSOC_EXHAUSTIVE)
    assert none == (0, 0)
    assert np.array_equal(ie, want_idx) and de.tobytes() == want_d2.tobytes(), (c, "exhaustive against the model")
    assert np.array_equal(ie[:len(c.pts)], [d[0] for d in sc.DECLARED[name]])
    i_s, ds, got = counted(torch, ctx, g, pts, api.ASSOC_SCREENED)
    print(name, "verified, fallback:", got, "declared:", c.counters())
    assert np.array_equal(i_s, ie) and ds.tobytes() == de.tobytes(), (c, "screened against exhaustive")
    assert got == c.counters(), (c, got, c.counters())
    if c.brute:
        opt("assoc_screen32", 1)
        opt("assoc_index_min", 1e12)
        ib, db, got = counted(torch, ctx, g, pts, api.ASSOC_BRUTE)
        assert np.array_equal(ib, ie) and db.tobytes() == de.tobytes(), (c, "brute, screened, against exhaustive")
        assert got == c.counters(), (c, "brute", got, c.counters())
    g.close()
