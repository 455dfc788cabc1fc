"""CPU tests of the octree ray entry points: they are exported, listed in voxhip.SYMBOLS, and refuse a null handle or null arguments
with VX_ERR_INVALID_ARG before anything touches a device."""
import ctypes as C

import numpy as np

INVALID_ARG = 1


def test_octree_trace_symbols_exported(vx):
    L = C.CDLL(vx.LIB_PATH)
    for n in ("vx_octree_trace", "vx_octree_trace_ex", "vx_octree_trace_ex_device"):
        assert hasattr(L, n) and n in vx.SYMBOLS
    assert hasattr(vx.Octree, "trace") and hasattr(vx.Octree, "trace_ex") and hasattr(vx.Octree, "trace_device")


def test_octree_trace_null_handle_and_args(vx):
    L = vx.lib()
    rays = np.zeros((4, 6), np.float32)
    t = np.zeros(4, np.float32)
    nh = C.c_uint64(7)
    assert L.vx_octree_trace(None, rays.ctypes.data, 4, np.float32(0.001), np.float32(1e4), t.ctypes.data, None, C.byref(nh)) == INVALID_ARG
    assert L.vx_octree_trace(None, None, 0, np.float32(0.001), np.float32(1e4), None, None, None) == INVALID_ARG
    a = vx.TraceArgs()
    a.rays, a.num_rays, a.t = rays.ctypes.data, 4, t.ctypes.data
    assert L.vx_octree_trace_ex(None, C.byref(a)) == INVALID_ARG
    assert L.vx_octree_trace_ex_device(None, C.byref(a)) == INVALID_ARG
    assert L.vx_octree_trace_ex(None, None) == INVALID_ARG
    assert L.vx_octree_trace_ex_device(None, None) == INVALID_ARG
    assert b"null" in L.vx_last_error()
