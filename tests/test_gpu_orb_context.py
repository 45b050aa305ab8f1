"""gl_orb_describe gives the bits of the FIRST call of a new context whatever the context has been through - the pass of
tests/context_pass.py for this module: after a larger call of itself (a larger pyramid and 4 096 key-points: the scratch block grows),
after mapping_pass_from_map, with every scratch block filled with 0x00 / 0xFF, and with the timers on.  This call DOES take scratch -
the blurred pyramid lies in the context's main block - so the poisoned legs hold it to writing every byte it reads."""
import functools

import pytest

from tests import orb_dev, orb_scenes
from tests.context_cases import BY_NAME
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)

pytestmark = pytest.mark.gpu

SIZES = {"tiny": dict(seed=0), "small": dict(seed=4000, size=(320, 240), n=4096)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return orb_scenes.random_scene(**SIZES[name])


def _describe(torch, ctx, name):
    s = _scene(name)
    return orb_dev.run(torch, ctx, [s, s], s["pattern"], s["blur_w"], s["scale_factor"])


CALLS = {"orb_describe": _describe}
PASS = Pass("orb", CALLS, small=dict.fromkeys(CALLS, "tiny"), larger=lambda name: (at(CALLS[name], "small"),),
            others=(BY_NAME["mapping_pass_from_map"].large,), prelude=(at(_describe, "small"),))


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
