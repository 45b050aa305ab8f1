"""Named non-default configurations for the parity tests: a camera, the hot-path parameters and the pyramid's
scale factor, each able to produce the api.Camera / api.Params pair of the HIP library, the orc_params of the C++
oracle and the Cam / Prm of oracle/numpy_ref.py FROM THE SAME VALUES.

The default configuration (cfg/v1.yaml = cfg/v2.yaml) is degenerate where it matters: fx == fy, tri_lambda2 ==
ba_lambda2, tri_check_str_chi2 == 1, a 1.2 level table, neighbor_dist_thresh == 2.5, one image size.  A kernel that
reads fx where fy is meant, one lambda for the other, a table hard-coded for 1.2 ... gives the same bits there.

Every intrinsic is a value that float represents exactly: the reference can only produce such values (config.h:38:
`extern float fx, fy, cx, cy`) and the matchers cast to float; other doubles are out of scope.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

F32 = np.float32
f32 = lambda x: float(np.float32(x))

PRM_FIELDS = ("neighbor_dist_thresh", "tri_lambda2", "tri_str_thresh", "ba_lambda2", "tri_check_str_chi2", "ba_first_as_prior")


def level_table(scale_factor):
    """frame::sigma2_inv for a scale factor, in float arithmetic the way init_config.hpp:60-79 builds it for 1.2."""
    sf, out = F32(1.0), [F32(1.0)]
    for _ in range(1, 8):
        sf = F32(sf * F32(scale_factor))
        out.append(F32(F32(1.0) / F32(sf * sf)))
    return np.array(out, dtype=np.float32)


DEFAULT_CAM = dict(fx=f32(435.2046959714599), fy=f32(435.2046959714599), cx=f32(367.4517211914062), cy=f32(252.2008514404297),
                   bf=f32(47.90639384423901), width=752, height=480)
DEFAULT_PRM = dict(neighbor_dist_thresh=2.5, tri_lambda2=400.0, tri_str_thresh=f32(0.0064), ba_lambda2=400.0, tri_check_str_chi2=1,
                   ba_first_as_prior=1)


class CamLike:
    """Plain attribute bag with the camera's fields: what synth.py, the oracle binding and numpy_ref all accept."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Config:
    def __init__(self, name, cam=None, prm=None, scale_factor=1.2, table_scale=None):
        """scale_factor: the argument the matchers take; table_scale: the pyramid gl_params.sigma2_inv is built for (None: the same
        one - a consistent host; the two differ only in the "default gl_params" mutation)"""
        self.name = name
        self.cam = dict(DEFAULT_CAM, **(cam or {}))
        self.prm = dict(DEFAULT_PRM, **(prm or {}))
        self.scale_factor = scale_factor
        self.table_scale = scale_factor if table_scale is None else table_scale
        self.sigma2_inv = level_table(self.table_scale)
        for k in ("fx", "fy", "cx", "cy", "bf"):
            assert self.cam[k] == f32(self.cam[k]), (name, k)
        for k in ("tri_lambda2", "tri_str_thresh", "ba_lambda2"):
            assert self.prm[k] == f32(self.prm[k]), (name, k)

    def __repr__(self):
        return self.name

    def replace(self, name=None, cam=None, prm=None, scale_factor=None):
        """A copy with some values changed (the mutations of the power checks)."""
        return Config(name or self.name + "*", dict(self.cam, **(cam or {})), dict(self.prm, **(prm or {})),
                      self.scale_factor if scale_factor is None else scale_factor)  # (the table follows the scale factor)

    def camlike(self):
        return CamLike(**self.cam)

    # ---- the HIP library
    def camera(self):
        from gmmloc_amd import api
        return api.Camera(**self.cam)

    def params(self, **kw):
        from gmmloc_amd import api
        return api.Params(sigma2_inv=(C.c_float * 8)(*[float(v) for v in self.sigma2_inv]), **dict(self.prm, **kw))

    # ---- the C++ oracle
    def orc_params(self, oracle, **kw):
        p = type(oracle.prm).from_buffer_copy(oracle.prm)
        for k, v in dict(self.prm, **kw).items():
            setattr(p, k, v)
        for i, v in enumerate(self.sigma2_inv):
            p.sigma2_inv[i] = float(v)
        return p

    # ---- the numpy restatement
    def np_cam(self):
        import numpy_ref as nr
        c = self.cam
        return nr.Cam(c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["width"], c["height"])

    def np_prm(self, **kw):
        import numpy_ref as nr
        p, v = nr.Prm(), dict(self.prm, **kw)
        p.neighbor_dist_thresh = float(v["neighbor_dist_thresh"])
        p.tri_lambda2, p.tri_str_thresh, p.ba_lambda2 = F32(v["tri_lambda2"]), F32(v["tri_str_thresh"]), F32(v["ba_lambda2"])
        p.tri_check_str_chi2, p.ba_first_as_prior = bool(v["tri_check_str_chi2"]), bool(v["ba_first_as_prior"])
        p.sigma2_inv = self.sigma2_inv.copy()
        return p


DEFAULT = Config("DEFAULT")

# anisotropic camera of another size, every parameter off its default, a 1.25 pyramid
ANISO = Config("ANISO",
               cam=dict(fx=f32(458.654), fy=f32(381.25), cx=f32(301.5), cy=f32(249.75), bf=f32(61.3), width=640, height=512),
               prm=dict(tri_lambda2=250.0, ba_lambda2=650.0, tri_str_thresh=f32(0.01), neighbor_dist_thresh=1.75),
               scale_factor=1.25)

# isotropic camera of another size and aspect with a large baseline term, default parameters: image size and grid effects alone
WIDE = Config("WIDE", cam=dict(fx=f32(718.856), fy=f32(718.856), cx=f32(607.1928), cy=f32(185.2157), bf=f32(386.1448), width=1241, height=376))

# default camera, the structure chi2 test switched off, the two lambdas apart; tri_str_thresh lowered from 0.0064 to 0.0005 so that
# ordinary points sit on both sides of tri_str_thresh * tri_lambda2 and the switched-off test is what decides for them
NOSTR = Config("NOSTR", prm=dict(tri_check_str_chi2=0, tri_lambda2=300.0, ba_lambda2=550.0, tri_str_thresh=f32(0.0005)))

CONFIGS = (ANISO, WIDE, NOSTR)


def _default_params(c):
    """The default gl_params under the configuration's camera: default scalar values AND the 1.2 table; the scale factor the
    matchers take as an argument of its own stays."""
    return Config(c.name + "*", c.cam, None, c.scale_factor, table_scale=1.2)


# the mutations of the power checks: what a kernel that reads the wrong field would compute
MUTATIONS = {
    "swap_fx_fy": lambda c: c.replace(cam=dict(fx=c.cam["fy"], fy=c.cam["fx"])),
    "swap_lambdas": lambda c: c.replace(prm=dict(tri_lambda2=c.prm["ba_lambda2"], ba_lambda2=c.prm["tri_lambda2"])),
    "default_params": _default_params,
    "scale_1.2": lambda c: c.replace(scale_factor=1.2),
}
