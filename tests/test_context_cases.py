"""The table of tests/context_cases.py is the whole public surface: every wrapper of gmmloc_amd.api that launches work on a context has a
case (so that tests/test_gpu_context_state.py runs it cold, after larger calls and on poisoned scratch), and every composite call is
held to the oracle when it runs cold.  No GPU needed."""
import inspect

from gmmloc_amd import api
from tests.context_cases import CASES, TIMING_CASES, BY_NAME

# wrappers that launch nothing on the context's stream or only allocate / describe
NOT_ENTRY_POINTS = {"local_map_lists", "ba_window_slab", "level_steps", "read_gmm_file", "write_gmm_file"}


def launching_wrappers():
    names = set()
    for name, fn in inspect.getmembers(api, inspect.isfunction):
        if name.startswith("_") or name in NOT_ENTRY_POINTS or fn.__module__ != api.__name__:
            continue
        if list(inspect.signature(fn).parameters)[:1] == ["ctx"]:
            names.add(name)
    names |= {"associate3d", "knn3d", "queryPoint", "search2d", "HostFramePath.track_frame"}
    for n in ("associate3d", "knn3d", "queryPoint", "search2d"):
        assert callable(getattr(api.GMM, n))
    assert callable(api.HostFramePath.track_frame)
    return names


def test_every_launching_wrapper_has_a_case():
    covered = {e for c in CASES for e in c.entries}
    want = launching_wrappers()
    assert len(want) >= 30
    assert want <= covered, sorted(want - covered)
    assert covered <= want, sorted(covered - want)


def test_every_composite_is_held_to_the_oracle_cold():
    checked = {c.name for c in CASES if c.check is not None}
    assert {"search_local_points", "track_frame_chain", "track_frame_chain_halves", "track_frame_chain_map", "joint_optimization_from_map",
            "mapping_pass_from_map", "track_frames_batch_shape", "track_frames_latency_shape"} <= checked
    assert all(n in BY_NAME for n in TIMING_CASES)
