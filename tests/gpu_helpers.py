"""What the GPU test modules share: the guard that ends a session at a device error, and the upload helpers.

Test infrastructure; nothing in the product imports it."""
import numpy as np
import pytest

_gmm = {}


@pytest.fixture(autouse=True)
def stop_on_device_error(gpu):
    """a HIP error met by a test is a finding: the session ends there, nothing more is started on the device.  Active in the modules
    that import it by name, and in no others"""
    yield
    try:
        gpu[0].cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, nothing more is started: %s" % e, returncode=3)


def T(torch, a, copy=False):
    """the array on the device; copy=True for read-only inputs (torch takes no read-only array as it stands)"""
    return torch.from_numpy(np.array(a, order="C") if copy else np.ascontiguousarray(a)).cuda()


def to_dev(torch, d, keys=None):
    """the dict (its `keys`, if given) with every ndarray uploaded, other values as they are and None dropped"""
    return {k: (T(torch, v) if isinstance(v, np.ndarray) else v) for k, v in d.items() if v is not None and (keys is None or k in keys)}


def gmm_of(ctx, mean, cov):
    """the GMM of (mean, cov), built at its first use"""
    from gmmloc_amd import api
    key = (mean.tobytes(), cov.tobytes())
    if key not in _gmm:
        _gmm[key] = api.GMM(ctx, mean, cov.reshape(-1, 9))
    return _gmm[key]
