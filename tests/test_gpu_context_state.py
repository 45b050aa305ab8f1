"""The same bits from every entry point whatever the context has been through.

A context hands a call whatever the previous call left in its scratch blocks (ctx_scratch never clears one), frees a block that has to
grow, and carries pipe_hint, the lds_limit / occupancy caches, the staging buffers, the timers' event pool and the registered statistics
buffers from call to call.  The other GPU tests share one warm context, so none of them sees an entry point that reads a word it never
wrote, a composite call that loses data when a block grows under it, a result that depends on what ran before, or bits that move with
timing or statistics switched on.  Here every case of tests/context_cases.py (one per public entry point) runs on contexts of this
module's own:

  R[c]  = the outputs of c.small as the FIRST call of a brand-new context (RL[c]: the same for c.large), computed once;
  cold      R[c] itself - for the composite calls and track_frames held to the oracle with the checker and the tolerances of the entry
            point's own test: the first time any of them runs cold, where every block it uses grows during the call;
  shrink    small, large, small, large on one new context: both small results equal R[c], both large results RL[c];
  after     on ONE context, `large` of every case, then `small` of every case in table order and in reverse order: each equals R[c]
            (for the pipelined local BA also the pipe_hint check: a many-cycle window precedes a few-cycle one in one direction and
            follows it in the other);
  poisoned  option test_scratch_fill = 0x00 / 0xFF on a context that has run `large` (every block filled at once), and on a new context
            before its first call (every block filled as it is allocated): `small` equals R[c].  0xFF reads as NaN in fp64 and fp32, -1
            in int32, "set" in a byte flag; 0x00 is a lucky fresh allocation.  No pattern reads as a large positive integer: realistic
            stale integers - the right type, in range for the larger problem - are what shrink and after supply;
  timing    with the timers on, and with the statistics buffers registered: R[c]; a de-registered buffer is not written again.

Equality is np.array_equal(..., equal_nan=True) on every key, same keys, shapes and dtypes."""
import pytest

from tests import context_pass
from tests.context_cases import BY_NAME, CASES, TIMING_CASES, close_context, new_context
from tests.context_pass import on_new_context, run, same, torch  # noqa: F401 (torch: the module's fixture)

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", CASES, ids=repr)


def first_call(torch, c, which="small"):
    return context_pass.first_call(torch, ("context_state", c.name, which), getattr(c, which))


@cases
def test_cold(torch, oracle, c):
    out = first_call(torch, c)
    if c.check is not None:
        c.check(oracle, out)


@cases
def test_shrink_and_regrow(torch, c):
    ref_s, ref_l = first_call(torch, c), first_call(torch, c, "large")
    ctx = new_context()
    try:
        for leg, fn, ref in (("small first", c.small, ref_s), ("large after small", c.large, ref_l), ("small after large", c.small, ref_s),
                             ("large again", c.large, ref_l)):
            same(run(fn, torch, ctx), ref, c.name, leg)
    finally:
        close_context(ctx)


def test_after_everything_else(torch):
    refs = [first_call(torch, c) for c in CASES]
    ctx = new_context()
    try:
        for c in CASES:  # the polluter round
            run(c.large, torch, ctx)
        for c, ref in zip(CASES, refs):
            same(run(c.small, torch, ctx), ref, c.name, "after every large call, table order")
        for c, ref in reversed(list(zip(CASES, refs))):
            same(run(c.small, torch, ctx), ref, c.name, "after every large call, reverse order")
    finally:
        close_context(ctx)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@cases
def test_poisoned(torch, c, v):
    ref = first_call(torch, c)
    ctx = new_context()
    try:
        run(c.large, torch, ctx)
        ctx.set_option("test_scratch_fill", v)  # every block the context holds, now
        assert ctx.get_option("test_scratch_fill") == v
        same(run(c.small, torch, ctx), ref, c.name, "blocks of the large call filled with 0x%02X" % v)
    finally:
        close_context(ctx)
    same(on_new_context(torch, c.small, fill=v), ref, c.name, "new context, blocks filled with 0x%02X as they are allocated" % v)


def test_scratch_fill_option(torch):
    """-1 by default; a byte or -1, nothing else; setting it back only stores the value"""
    from gmmloc_amd import api
    ctx = new_context()
    try:
        assert ctx.get_option("test_scratch_fill") == -1
        ctx.set_option("test_scratch_fill", 0xA5)  # (no block yet: nothing to fill)
        with pytest.raises(api.GLError):
            ctx.set_option("test_scratch_fill", 256)
        assert ctx.get_option("test_scratch_fill") == 0xA5
        ctx.set_option("test_scratch_fill", -1)
        assert ctx.get_option("test_scratch_fill") == -1
    finally:
        close_context(ctx)


def test_timing_and_statistics(torch):
    from gmmloc_amd import api
    picked = [BY_NAME[n] for n in TIMING_CASES]
    refs = [first_call(torch, c) for c in picked]
    ctx = new_context()
    try:
        ctx.timing(True)
        for _ in range(2):  # (the second round takes its events from the pool)
            for c, ref in zip(picked, refs):
                same(run(c.small, torch, ctx), ref, c.name, "timers on")
        assert ctx.timing_read(api.TIMER_BA)[1] > 0 and ctx.timing_read(api.TIMER_REFINE_POSE)[1] > 0 and ctx.timing_read(api.TIMER_ASSOC)[1] > 0
        ctx.timing(False)
        SENT = -77
        trials, iters = torch.full((64,), SENT, dtype=torch.int32).cuda(), torch.full((64,), SENT, dtype=torch.int32).cuda()
        edges = torch.full((64, 2), SENT, dtype=torch.int32).cuda()
        ctx.set_stats_buffer(trials, iters)
        ctx.set_edge_stats_buffer(edges)
        for c, ref in zip(picked, refs):
            same(run(c.small, torch, ctx), ref, c.name, "statistics buffers registered")
            if c.name == "track_frames_batch_shape":  # (three frames: the refine writes their trial counts and edge sums)
                assert (trials[:3] > 0).all() and (iters[:3] > 0).all() and (edges[:3] > 0).all(), "the registered buffers were never written"
        ctx.set_stats_buffer(None)  # n = 0
        ctx.set_edge_stats_buffer(None)
        for t in (trials, iters, edges):
            t.fill_(SENT)
        for c, ref in zip(picked, refs):
            same(run(c.small, torch, ctx), ref, c.name, "statistics buffers de-registered")
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in (trials, iters, edges)), "a de-registered statistics buffer was written"
    finally:
        close_context(ctx)
