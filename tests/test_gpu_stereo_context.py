"""gl_stereo_matches gives the bits of the FIRST call of a new context whatever the context has been through - the pass of
tests/context_pass.py for this module: after a larger call of itself (4 096 key-points a side: a workgroup's LDS nearly full where the
small call leaves most of it untouched), after mapping_pass_from_map, with every scratch block filled with 0x00 / 0xFF, and with the
timers on.  The call takes no scratch block; the pass holds it to that."""
import functools

import pytest

from tests import stereo_dev, stereo_scenes
from tests.context_cases import BY_NAME
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)

pytestmark = pytest.mark.gpu

SIZES = {"tiny": dict(seed=0), "small": dict(seed=4000, size=(320, 240), nfeat=4096)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return stereo_scenes.random_scene(**SIZES[name])


def _stereo(torch, ctx, name):
    s = _scene(name)
    return stereo_dev.run(torch, ctx, s["cam"], s["scale_factor"], [s["frame"], s["frame"]])


CALLS = {"stereo_matches": _stereo}
PASS = Pass("stereo", CALLS, small=dict.fromkeys(CALLS, "tiny"), larger=lambda name: (at(CALLS[name], "small"),),
            others=(BY_NAME["mapping_pass_from_map"].large,), prelude=(at(_stereo, "small"),))


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
