"""gl_orb_detect and the composite orb.extract give the bits of the FIRST call of a new context whatever the context has been through -
the pass of tests/context_pass.py for this module: after a larger call of itself (more pixels, more candidate slots: the scratch block
grows), after mapping_pass_from_map, with every scratch block filled with 0x00 / 0xFF, and with the timers on.  Detect keeps the score
map, the cell counts, the candidate lists and the levels' results in the context's main block - and with 16 384 candidate slots the
octree's working set too - so the poisoned legs hold it to writing every byte it reads."""
import functools

import numpy as np
import pytest

from tests import orb_detect_dev as dev, orb_detect_ref as ref, orb_scenes
from tests.context_cases import BY_NAME
from tests.context_pass import Pass, after_legs, at, poisoned, timers_on, torch  # noqa: F401 (torch: the module's fixture)

pytestmark = pytest.mark.gpu

SIZES = {"tiny": dict(seed=0, size=(160, 120), nlevels=3, nfeatures=200, cap=2048), "tiny-scratch": dict(seed=0, size=(160, 120), nlevels=3, nfeatures=200, cap=16384),
         "small": dict(seed=4000, size=(320, 240), nlevels=6, nfeatures=1500, cap=8192)}


@functools.lru_cache(maxsize=None)
def _image(name):
    s = SIZES[name]
    return dev.scene(s["seed"], s["size"])


def _detect(torch, ctx, name):
    s = SIZES[name]
    levels = dev.IMAGES[dev.register(("context", name), ref.pyramid(_image(name), s["nlevels"]))]
    N = sum(ref.level_bound(l.shape[1], l.shape[0], n) for l, n in zip(levels, ref.features_per_level(s["nfeatures"], s["nlevels"])))
    return dev.run(torch, ctx, [levels, levels], s["nfeatures"], N, s["cap"])


def _extract(torch, ctx, name):
    from gmmloc_amd import orb
    s = SIZES[name]
    d = torch.device("cuda:0")
    im = torch.from_numpy(np.stack([_image(name)] * 2)).to(d)
    pyr, det, des = orb.extract(ctx, im, torch.from_numpy(orb_scenes.PATTERN).to(d), nfeatures=s["nfeatures"], nlevels=s["nlevels"], cand_cap=s["cap"])
    ctx.synchronize()
    out = {"pyramid": pyr.data.cpu().numpy()}
    out.update({"det_" + k: v.cpu().numpy() for k, v in det.items()})
    out.update({"des_" + k: v.cpu().numpy() for k, v in des.items()})
    return out


CALLS = {"orb_detect": _detect, "orb_detect_scratch": _detect, "orb_extract": _extract}
PASS = Pass("orb_detect", CALLS, small={"orb_detect": "tiny", "orb_detect_scratch": "tiny-scratch", "orb_extract": "tiny"},
            larger=lambda name: (at(CALLS[name], "small"),), others=(BY_NAME["mapping_pass_from_map"].large,), prelude=(at(_detect, "small"),))


@pytest.mark.parametrize("name", list(CALLS))
def test_after_larger_calls_and_the_mapping_pass(torch, name):
    after_legs(torch, PASS, name)


@pytest.mark.parametrize("v", [0x00, 0xFF], ids=["0x00", "0xFF"])
@pytest.mark.parametrize("name", list(CALLS))
def test_poisoned_scratch(torch, name, v):
    poisoned(torch, PASS, name, v)


def test_timers_on(torch):
    timers_on(torch, PASS)
