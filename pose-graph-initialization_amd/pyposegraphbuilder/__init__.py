"""pyposegraphbuilder -- MI355X-native pairwise relative-pose engine.

The name is the reference's (empty) Python package (src/pyposegraphbuilder/__init__.py:1).
All compute runs in libpgi.so (HIP, gfx950); there is no CPU fallback.
"""
from . import synthetic  # noqa: F401
from ._lib import EDGE_DTYPE, PgiError, default_params  # noqa: F401
from ._lib import (TRI_BEHIND, TRI_DEGENERATE, TRI_LOW_PARALLAX, TRI_OK, TRI_REPROJ, TRI_STATUS_COUNT,  # noqa: F401
                   TRI_STATUS_NAMES, TRI_TOO_FEW)
from ._lib import BA_STOP_EMPTY, BA_STOP_FTOL, BA_STOP_ITERS, BA_STOP_LAMBDA, BundleParams, BundleReport  # noqa: F401
from ._lib import EDGE_INCONSISTENT, EDGE_OK, CycleParams, CycleSummary  # noqa: F401


def __getattr__(name):  # torch-dependent parts are imported lazily
    if name in ("Engine", "DeviceTracklets", "Triangulation", "BundleResult"):
        from . import engine
        return getattr(engine, name)
    if name in ("PoseGraphBuilder", "findEssentialMatrix", "bindProcessToDeviceNode"):
        from . import builder
        return getattr(builder, name)
    raise AttributeError(name)
