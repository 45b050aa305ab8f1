"""gmmloc_amd -- MI355X-native hot path of GMMLoc behind a C-ABI.

The product is ``libgmmloc_hip.so`` (hand-written HIP for gfx950, built in-tree by
``__graft_entry__.build()``); this package is the thin Python host side used by
the tests and the benchmark: ctypes bindings (``_lib``) and a mirror of the
reference's operator interface (``api``).  There is NO CPU fallback: importing
``api`` without the shared library raises, and every call needs a GPU.
"""
from .api import (  # noqa: F401
    Camera,
    Params,
    Context,
    GMM,
    GLError,
    ASSOC_BRUTE,
    ASSOC_KNN5_EUCLID,
    ASSOC_EXHAUSTIVE,
    optimize_current_pose,
    track_frames,
    track_frames_anchored,
)
from .map_grow import map_add, map_fuse, fuse_observations_from_map, map_views, process_key_frame_from_map  # noqa: F401
from . import bow  # noqa: F401
from . import stereo  # noqa: F401
from .stereo import stereo_matches  # noqa: F401
from . import orb  # noqa: F401
from .bow import Vocabulary  # noqa: F401
from .map_stats import map_stats_alloc, track_frame_with_stats, remove_map_points_from_map  # noqa: F401
from .frame_step import track_frame_step  # noqa: F401
