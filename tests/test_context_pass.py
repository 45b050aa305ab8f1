"""The shared context pass (tests/context_pass.py) itself, on the CPU: `same` and `run` decide as they say, and the three legs make
their calls, fills, timing switch and closes in the stated order - on a recording stand-in for the context, with no device."""
import numpy as np
import pytest

from tests import context_pass as P


def raising(exc):
    def fn(torch, ctx):
        raise exc
    return fn


def test_same_and_run():
    ref = dict(a=np.array([1.0, np.nan, 3.0]), b=np.arange(6, dtype=np.int32).reshape(2, 3))
    good = {k: v.copy() for k, v in ref.items()}
    P.same(good, ref, "c", "l")  # (NaN against NaN is equal)
    one = ref["b"].copy()
    one[1, 1] += 1
    rejected = {"a missing key": dict(a=ref["a"]), "an extra key": dict(good, c=np.zeros(1)), "a dtype change": dict(good, b=ref["b"].astype(np.int64)),
                "a shape change": dict(good, b=ref["b"].reshape(3, 2)), "one differing element": dict(good, b=one),
                "NaN against a number": dict(good, a=np.array([1.0, 2.0, 3.0])), "a number against NaN": dict(good, a=np.array([np.nan, np.nan, 3.0]))}
    for what, got in rejected.items():
        with pytest.raises(AssertionError):
            P.same(got, ref, "c", "l")
            pytest.fail("same accepted " + what)
    with pytest.raises(AssertionError, match="case c, leg l, output b: 1 of 6 elements differ"):
        P.same(rejected["one differing element"], ref, "c", "l")

    assert P.run(lambda torch, ctx: (torch, ctx), 1, 2) == (1, 2)
    with pytest.raises(pytest.exit.Exception) as e:
        P.run(raising(RuntimeError("an illegal memory access was encountered")), None, None)
    assert e.value.returncode == 3
    with pytest.raises(RuntimeError, match="sizes do not match"):
        P.run(raising(RuntimeError("sizes do not match")), None, None)


class Recorder:
    """new_context / close_context of the pass, and the context's set_option / timing, as entries of one log"""

    def __init__(self, monkeypatch):
        self.log, self.made = [], 0
        monkeypatch.setattr(P, "new_context", self.new)
        monkeypatch.setattr(P, "close_context", lambda ctx: self.log.append(("close", ctx.n)))
        monkeypatch.setattr(P, "_first", {})

    def new(self):
        ctx = type("Ctx", (), dict(n=self.made, set_option=lambda c, k, v: self.log.append(("option", c.n, k, v)),
                                   timing=lambda c, on: self.log.append(("timing", c.n, on))))()
        self.made += 1
        self.log.append(("new", ctx.n))
        return ctx

    def call(self, name):
        def fn(torch, ctx, size):
            self.log.append((name, size, ctx.n))
            return dict(out=np.array([len(name)]))
        return fn

    def take(self):
        log, self.log = self.log, []
        return log


def test_the_three_legs_on_a_recording_context(monkeypatch):
    r = Recorder(monkeypatch)
    calls = dict(a=r.call("a"), b=r.call("b"))
    p = P.Pass("fake", calls, small=dict(a="s", b=None), larger=lambda name: (P.at(calls[name], "L"), P.at(r.call("part"), "L")),
               others=(P.at(r.call("other"), "L"),), prelude=(P.at(r.call("pre"), "L"),), legs=("second", "third"))
    FILL = "test_scratch_fill"
    P.after_legs(None, p, "a")  # context 0 makes the reference, once
    assert r.take() == [("new", 0), ("a", "s", 0), ("close", 0),
                        ("new", 1), ("a", "s", 1), ("a", "L", 1), ("part", "L", 1), ("a", "s", 1), ("other", "L", 1), ("a", "s", 1), ("close", 1)]
    P.after_legs(None, p, "a")
    assert r.take() == [("new", 2), ("a", "s", 2), ("a", "L", 2), ("part", "L", 2), ("a", "s", 2), ("other", "L", 2), ("a", "s", 2), ("close", 2)]
    P.poisoned(None, p, "b", 0xFF)
    assert r.take() == [("new", 3), ("b", None, 3), ("close", 3),
                        ("new", 4), ("pre", "L", 4), ("option", 4, FILL, 0xFF), ("b", None, 4), ("close", 4),
                        ("new", 5), ("option", 5, FILL, 0xFF), ("b", None, 5), ("close", 5)]
    P.timers_on(None, p)
    assert r.take() == [("new", 6), ("timing", 6, True), ("a", "s", 6), ("b", None, 6), ("a", "s", 6), ("b", None, 6), ("close", 6)]
    assert sorted(P._first) == [("fake", "a", "s"), ("fake", "b", None)] and not any(v["out"].flags.writeable for v in P._first.values())

    # a call whose result moves after its first call: every leg raises inside its context, and closes it
    seen = []

    def moving(torch, ctx, size):
        seen.append(ctx.n)
        return dict(out=np.array([len(seen) > 1]))
    q = P.Pass("moving", dict(m=moving), small=dict(m="s"), larger=lambda name: (), others=(), prelude=())
    for leg in (lambda: P.after_legs(None, q, "m"), lambda: P.poisoned(None, q, "m", 0x00), lambda: P.timers_on(None, q)):
        with pytest.raises(AssertionError, match="case m, leg .*, output out: 1 of 1 elements differ"):
            leg()
        log = r.take()
        assert log[-1][0] == "close" and [e[1] for e in log if e[0] == "new"] == [e[1] for e in log if e[0] == "close"], log
