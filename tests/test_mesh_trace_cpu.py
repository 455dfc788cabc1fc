"""CPU tests of the triangle ray queries (vx_bvh_*): the entry points are exported and listed in voxhip.SYMBOLS, refuse a null handle or
null arguments with VX_ERR_INVALID_ARG before anything touches a device, and the numpy restatement of the contract (tests/mesh_ref.py)
behaves as include/voxhip.h pins it on hand-made cases."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402

INVALID_ARG = 1
BVH_SYMBOLS = ("vx_bvh_build", "vx_bvh_build_into", "vx_bvh_num_triangles", "vx_bvh_num_nodes", "vx_bvh_bytes", "vx_bvh_height",
               "vx_bvh_num_ill_conditioned", "vx_bvh_root_bounds", "vx_bvh_nodes", "vx_bvh_leaf_triangles", "vx_bvh_nodes_device", "vx_bvh_trace_ex_device",
               "vx_bvh_trace_ex", "vx_bvh_trace", "vx_bvh_free", "vx_device_allocations")

# two triangles of the unit square in z = 0 sharing the edge (1,0,0)-(0,1,0)
SQ_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
SQ_T = np.int32([[0, 1, 2], [1, 3, 2]])


def ray(o, d):
    return np.float32([list(o) + list(d)])


def test_bvh_symbols_exported(vx):
    L = C.CDLL(vx.LIB_PATH)
    for n in BVH_SYMBOLS:
        assert hasattr(L, n) and n in vx.SYMBOLS, n
    for m in ("trace", "trace_ex", "trace_device", "build_into", "nodes", "root_bounds", "free"):
        assert hasattr(vx.Bvh, m)
    assert hasattr(vx.Mesh, "bvh")


def test_bvh_null_handle_and_args(vx):
    L = vx.lib()
    rays = np.zeros((4, 6), np.float32)
    t = np.zeros(4, np.float32)
    nh = C.c_uint64(7)
    h = C.c_void_p()
    assert L.vx_bvh_build(None, 0, None, C.byref(h)) == INVALID_ARG
    assert L.vx_bvh_build_into(None, None) == INVALID_ARG
    assert L.vx_bvh_trace(None, rays.ctypes.data, 4, np.float32(0.001), np.float32(1e4), t.ctypes.data, None, C.byref(nh)) == INVALID_ARG
    assert L.vx_bvh_trace(None, None, 0, np.float32(0.001), np.float32(1e4), None, None, None) == INVALID_ARG
    a = vx.BvhTraceArgs()
    a.base.rays, a.base.num_rays, a.base.t = rays.ctypes.data, 4, t.ctypes.data
    assert L.vx_bvh_trace_ex(None, C.byref(a)) == INVALID_ARG
    assert L.vx_bvh_trace_ex_device(None, C.byref(a)) == INVALID_ARG
    assert L.vx_bvh_trace_ex(None, None) == INVALID_ARG
    assert L.vx_bvh_trace_ex_device(None, None) == INVALID_ARG
    mn, mx = (C.c_float * 3)(), (C.c_float * 3)()
    assert L.vx_bvh_root_bounds(None, mn, mx) == INVALID_ARG
    assert L.vx_bvh_nodes(None, None, 0, None) == INVALID_ARG
    assert L.vx_bvh_leaf_triangles(None, None, 0) == INVALID_ARG
    assert b"null" in L.vx_last_error()
    assert L.vx_bvh_num_triangles(None) == 0 and L.vx_bvh_num_nodes(None) == 0 and L.vx_bvh_bytes(None) == 0
    assert L.vx_bvh_num_ill_conditioned(None) == 0
    L.vx_bvh_free(None)


def test_ref_shared_edge_reports_lower_index():
    r = ray((0.5, 0.5, 1.0), (0.0, 0.0, -1.0))        # through the midpoint of the shared edge
    for tris in (SQ_T, SQ_T[::-1].copy()):
        for k in range(2):                            # each triangle alone accepts the ray at t = 1
            t, p, _ = mesh_ref.closest(SQ_V, tris[k:k + 1], r)
            assert t[0] == 1.0 and p[0] == 0
        t, p, b = mesh_ref.closest(SQ_V, tris, r)
        assert t[0] == 1.0 and p[0] == 0
        _, _, b0 = mesh_ref.closest(SQ_V, tris[:1], r)
        assert np.array_equal(b, b0)


def test_ref_shared_vertex():
    # a fan of eight triangles around the vertex (0, 0, 0) (integer ring: every t is exact), in several orders
    ring = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    v = np.float32([[0, 0, 0]] + [[x, y, 0] for x, y in ring])
    t = np.int32([[0, 1 + i, 1 + (i + 1) % 8] for i in range(8)])
    r = ray((0.0, 0.0, 2.0), (0.0, 0.0, -1.0))
    for perm in (np.arange(8), np.arange(8)[::-1], np.int32([3, 1, 5, 7, 0, 2, 6, 4])):
        tt = t[perm]
        single = [mesh_ref.closest(v, tt[k:k + 1], r)[0][0] for k in range(8)]
        assert all(s == 2.0 for s in single)           # closed vertices: every triangle of the fan accepts it
        th, p, b = mesh_ref.closest(v, tt, r)
        assert th[0] == 2.0 and p[0] == 0
        assert b[0, 0] == 0.0 and b[0, 1] == 0.0       # the vertex is v0 of every fan triangle


def test_ref_edge_on_ray_misses():
    r = ray((-1.0, 0.25, 0.0), (1.0, 0.0, 0.0))       # in the plane of the square: det == 0
    t, p, b = mesh_ref.closest(SQ_V, SQ_T, r)
    assert t[0] == -1.0 and p[0] == mesh_ref.MISS and not b.any()
    assert mesh_ref.any_hit(SQ_V, SQ_T, r)[0] == 0


def test_ref_degenerate_triangle_misses():
    v = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0, 0]])
    for tri in ([0, 1, 2], [0, 0, 0], [0, 1, 1], [0, 3, 1]):
        for r in (ray((0.5, 0.0, 1.0), (0.0, 0.0, -1.0)), ray((0.5, 1.0, 0.0), (0.0, -1.0, 0.0)), ray((0.5, 1.0, 1.0), (0.0, -0.7071, -0.7071))):
            t, p, _ = mesh_ref.closest(v, np.int32([tri]), r)
            assert t[0] == -1.0 and p[0] == mesh_ref.MISS


def test_ref_interval_bounds_are_closed():
    r = ray((0.25, 0.25, 1.0), (0.0, 0.0, -1.0))      # t = 1 exactly
    assert mesh_ref.closest(SQ_V, SQ_T, r, tmin=1.0)[0][0] == 1.0
    assert mesh_ref.closest(SQ_V, SQ_T, r, tmax=1.0)[0][0] == 1.0
    assert mesh_ref.closest(SQ_V, SQ_T, r, tmin=1.0, tmax=1.0)[0][0] == 1.0
    assert mesh_ref.closest(SQ_V, SQ_T, r, tmax=np.nextafter(np.float32(1.0), np.float32(0.0)))[0][0] == -1.0
    assert mesh_ref.closest(SQ_V, SQ_T, r, tmin=np.nextafter(np.float32(1.0), np.float32(2.0)))[0][0] == -1.0
    tpr = np.float32([1.0])
    assert mesh_ref.any_hit(SQ_V, SQ_T, r, tmax_per_ray=tpr)[0] == 1
    assert mesh_ref.any_hit(SQ_V, SQ_T, r, tmax_per_ray=tpr * np.float32(0.5))[0] == 0


def test_ref_origin_on_triangle_misses():
    r = ray((0.25, 0.25, 0.0), (0.0, 0.0, -1.0))      # t = 0: not t > 0, whatever tmin is
    for tmin in (0.001, 0.0, -1.0):
        assert mesh_ref.closest(SQ_V, SQ_T, r, tmin=tmin)[0][0] == -1.0
        assert mesh_ref.any_hit(SQ_V, SQ_T, r, tmin=tmin)[0] == 0


def test_ref_zero_direction_components():
    base = mesh_ref.closest(SQ_V, SQ_T, ray((0.25, 0.25, 1.0), (0.0, 0.0, -1.0)))
    for d in ((-0.0, 0.0, -1.0), (0.0, -0.0, -1.0), (-0.0, -0.0, -1.0)):
        got = mesh_ref.closest(SQ_V, SQ_T, ray((0.25, 0.25, 1.0), d))
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
    assert base[0][0] == 1.0 and base[1][0] == 0
    assert mesh_ref.closest(SQ_V, SQ_T, ray((0.25, 0.25, 1.0), (0.0, 0.0, 0.0)))[0][0] == -1.0   # no direction: det == 0
    # a wall x = 0.5 hit by a ray with a zero y component
    wv = np.float32([[0.5, 0, 0], [0.5, 1, 0], [0.5, 0, 1]])
    t, p, b = mesh_ref.closest(wv, np.int32([[0, 1, 2]]), ray((0.0, 0.25, 0.25), (1.0, 0.0, 0.0)))
    assert t[0] == 0.5 and p[0] == 0 and b[0, 0] == 0.25 and b[0, 1] == 0.25
    n = mesh_ref.normals(wv, np.int32([[0, 1, 2]]), p)
    assert np.allclose(n[0], [1.0, 0.0, 0.0])
