"""CPU tests of device frames (vx_render_*): the entry points are exported and listed in voxhip.SYMBOLS, argument errors come back as
VX_ERR_INVALID_ARG with their message before anything touches a device, a frame without a device is VX_ERR_NO_DEVICE, and the numpy
restatement of the shading stage (tests/render_ref.py) gives hand-worked colours on single pixels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref  # noqa: E402

INVALID_ARG, NO_DEVICE = 1, 6
F = np.float32
RENDER_SYMBOLS = ("vx_render_create", "vx_render_refresh", "vx_render_frame_device", "vx_render_frame", "vx_render_free")


def test_render_symbols_exported(vx):
    L = C.CDLL(vx.LIB_PATH)
    for n in RENDER_SYMBOLS:
        assert hasattr(L, n) and n in vx.SYMBOLS, n
    for m in ("render", "render_host", "refresh", "free"):
        assert hasattr(vx.Renderer, m)


def _args(vx, w=4, h=3, light=None, rgba=True):
    vi = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    a = vx.RenderArgs()
    a.view_inverse, a.proj_inverse, a.width, a.height = vi, vi, w, h
    buf = np.zeros(max(w * h, 1), np.uint32)
    if rgba:
        a.rgba = buf.ctypes.data
    if light is not None:
        a.light = C.pointer(light)
    return a, (vi, buf, light)


def _err(vx, status, text):
    assert status == INVALID_ARG
    assert text in vx.lib().vx_last_error().decode(), vx.lib().vx_last_error()


def test_render_create_argument_errors(vx):
    L = vx.lib()
    h = C.c_void_p()
    _err(vx, L.vx_render_create(None, C.byref(h)), "null")
    d = vx.RenderDesc()
    _err(vx, L.vx_render_create(C.byref(d), None), "null")
    _err(vx, L.vx_render_create(C.byref(d), C.byref(h)), "exactly one voxel source")
    d.grid, d.octree = C.c_void_p(16), C.c_void_p(32)       # never dereferenced: the pointer checks come first
    _err(vx, L.vx_render_create(C.byref(d), C.byref(h)), "exactly one voxel source")
    d.octree = None
    d.bvh = C.c_void_p(48)
    _err(vx, L.vx_render_create(C.byref(d), C.byref(h)), "bvh and mesh go together")
    d.bvh, d.mesh = None, C.c_void_p(64)
    _err(vx, L.vx_render_create(C.byref(d), C.byref(h)), "bvh and mesh go together")
    assert not h.value


def test_render_frame_argument_errors(vx):
    L = vx.lib()
    for fn in (L.vx_render_frame_device, L.vx_render_frame):
        _err(vx, fn(None, None), "null")
        a, keep = _args(vx, rgba=False)
        _err(vx, fn(None, C.byref(a)), "null")
        for w, h in ((0, 3), (4, 0)):
            a, keep = _args(vx, w, h)
            _err(vx, fn(None, C.byref(a)), "zero width or height")
        for t in (2, -1):
            lt = vx.RenderLight()
            lt.position = (C.c_float * 3)(1, 2, 3)
            lt.intensity, lt.type = 1.0, t
            a, keep = _args(vx, light=lt)
            _err(vx, fn(None, C.byref(a)), "light type")
        a, keep = _args(vx)
        st = fn(None, C.byref(a))
        assert st == (INVALID_ARG if vx.device_count() > 0 else NO_DEVICE)
    _err(vx, L.vx_render_refresh(None), "null")
    L.vx_render_free(None)


def test_render_no_device(vx):
    """Without a device neither a scene nor a frame computes anything: VX_ERR_NO_DEVICE, no CPU path."""
    if vx.device_count() > 0:
        pytest.skip("a GPU is present")
    L = vx.lib()
    d = vx.RenderDesc()
    d.grid = C.c_void_p(16)                                  # the device check precedes every use of the handles
    h = C.c_void_p()
    assert L.vx_render_create(C.byref(d), C.byref(h)) == NO_DEVICE and not h.value
    a, keep = _args(vx)
    assert L.vx_render_frame_device(C.c_void_p(16), C.byref(a)) == NO_DEVICE
    assert L.vx_render_frame(C.c_void_p(16), C.byref(a)) == NO_DEVICE
    assert b"no HIP device" in L.vx_last_error()


# ---- render_ref on single pixels with hand-worked colours ------------------------------------------------------------------------
DOWN, UP = F([[0, -1, 0]]), F([[0, 1, 0]])


def one(kind, normal, L, dist, sv=0, sm=0, light=(F([0, 20, 0]), F(100), 0), mat=None):
    """one pixel looking straight down; kind 1 = voxel (normal = cube normal), 2 = triangle (normal = geometric normal)"""
    k = np.uint8([kind])
    m = None if mat is None else render_ref.per_pixel_materials(mat, [0], 1)
    vm, mm = (m, None) if kind == 1 else (None, m)
    return render_ref.shade(DOWN, k, F([normal]), F([normal]), F([L]), F([dist]), np.uint8([sv]), np.uint8([sm]), light, vm, mm)


def test_render_ref_floor_under_point_light():
    # floor at the origin, light 20 above, intensity 100: li = 100 / 400 = 0.25; MaterialObj{} diffuse (1, 1, 0), illum 0
    # lit: c = 0.25 -> 0.25^(1/2.2) = 0.5325 -> 135.8 -> 136;  blue: 0
    rgba, sh = one(1, [0, 1, 0], [0, 1, 0], 20.0)
    assert rgba[0].tolist() == [136, 136, 0, 255] and sh[0] == 0
    # shadowed (either query): c = 0.25 * 0.3 = 0.075 -> 0.3081 -> 78.6 -> 79
    for sv, sm in ((1, 0), (0, 1), (1, 1)):
        rgba, sh = one(1, [0, 1, 0], [0, 1, 0], 20.0, sv, sm)
        assert rgba[0].tolist() == [79, 79, 0, 255] and sh[0] == 1
    # facing away (light below the floor): no diffuse, no ambient at illum 0 -> black; the shadow flag is not read
    rgba, sh = one(1, [0, 1, 0], [0, -1, 0], 20.0, 1, 1)
    assert rgba[0].tolist() == [0, 0, 0, 255] and sh[0] == 0
    # a triangle floor gives the same lit and shadowed colours
    assert one(2, [0, 1, 0], [0, 1, 0], 20.0)[0][0].tolist() == [136, 136, 0, 255]
    assert one(2, [0, -1, 0], [0, 1, 0], 20.0, 0, 1)[0][0].tolist() == [79, 79, 0, 255]   # the normal is turned toward the ray


def test_render_ref_unlit_attenuation_asymmetry():
    # illum 1 material with ambient 0.4, light behind the surface: c = li * att * 0.4 with att 0.3 for a voxel, 1 for a triangle
    mat = np.zeros(1, dtype=[("ambient", F, 3), ("diffuse", F, 3), ("specular", F, 3), ("shininess", F), ("illum", np.int32)])
    mat["ambient"], mat["diffuse"], mat["illum"] = 0.4, 0.5, 1
    # li = 0.25: voxel 0.03 -> 0.03^(1/2.2) = 0.2033 -> 51.8 -> 52; triangle 0.1 -> 0.3511 -> 89.5 -> 90
    assert one(1, [0, 1, 0], [0, -1, 0], 20.0, mat=mat)[0][0].tolist() == [52, 52, 52, 255]
    assert one(2, [0, 1, 0], [0, -1, 0], 20.0, mat=mat)[0][0].tolist() == [90, 90, 90, 255]


def test_render_ref_directional_light():
    # type 1: L = normalize(position), intensity not divided (0.5): c = 0.5 -> 0.7297 -> 186.1 -> 186; the shadow ray's tMax is 100000
    light = (F([0, 2, 0]), F(0.5), 1)
    assert one(1, [0, 1, 0], [0, 1, 0], 100000.0, light=light)[0][0].tolist() == [186, 186, 0, 255]
    kind = np.uint8([1])
    rays, dist = render_ref.shadow_rays(F([0, 5, 0]), DOWN, kind, F([5.0]), light=light)
    assert rays[0].tolist() == [0, 0, 0, 0, 1, 0] and dist[0] == 100000


def test_render_ref_specular_illum2():
    # diffuse 0.5 + ambient 0.1, specular 1, shininess 4: kE = 6 / (2 pi) = 0.95493, V = R = up -> sp = kE; li = 0.25
    # c = 0.25 * (0.6 + 0.95493) = 0.38873 -> 0.6509 -> 165.97 -> 166;  shadowed: no specular, 0.25 * 0.3 * 0.6 = 0.045 -> 0.2437 -> 62
    mat = np.zeros(1, dtype=[("ambient", F, 3), ("diffuse", F, 3), ("specular", F, 3), ("shininess", F), ("illum", np.int32)])
    mat["ambient"], mat["diffuse"], mat["specular"], mat["shininess"], mat["illum"] = 0.1, 0.5, 1.0, 4.0, 2
    assert one(1, [0, 1, 0], [0, 1, 0], 20.0, mat=mat)[0][0].tolist() == [166, 166, 166, 255]
    assert one(1, [0, 1, 0], [0, 1, 0], 20.0, sv=1, mat=mat)[0][0].tolist() == [62, 62, 62, 255]


def test_render_ref_miss_and_point_shadow_ray():
    rgba, sh = render_ref.shade(DOWN, np.uint8([0]), F([[0, 0, 0]]), F([[0, 0, 0]]), F([[0, 1, 0]]), F([1.0]), np.uint8([1]), None)
    assert rgba[0].tolist() == [230, 230, 230, 255] and sh[0] == 0          # rmiss 0.8, gamma'd: 0.9036 -> 230.4 -> 230
    # point light straight above a voxel hit at t = 5 from (0, 5, 0): origin (0, 0, 0), L = up, tMax = 20
    rays, dist = render_ref.shadow_rays(F([0, 5, 0]), DOWN, np.uint8([1]), F([5.0]), light=(F([0, 20, 0]), F(100), 0))
    assert rays[0].tolist() == [0, 0, 0, 0, 1, 0] and dist[0] == 20
    # triangle hit: the light vector starts at the barycentric position, the ray at org + dir * t
    v, t = F([[-1, 0, -1], [1, 0, -1], [0, 0, 1]]), np.int32([[0, 1, 2]])
    rays, dist = render_ref.shadow_rays(F([0, 5, 0]), DOWN, np.uint8([2]), F([-1.0]), F([5.0]), np.uint32([0]), F([[0.0, 0.0]]), v, t,
                                        light=(F([-1, 20, -1]), F(100), 0))
    assert rays[0, :3].tolist() == [0, 0, 0] and rays[0, 3:].tolist() == [0, 1, 0] and dist[0] == 20
