"""CPU tests of the ray queries' binding: voxhip._ray_batch fills the batch of each of the six argument structures as written out by hand
here, voxhip._outputs hands out the documented shapes and dtypes and refuses what a structure does not have, and every vx_*_trace_ex* /
vx_*_trace_multi* entry point and every grid field entry point refuses a null handle before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

INVALID_ARG = 1
RAYS = np.float32([[0, 0, 5, 0, 0, -1], [1, 2, 3, 0, 1, 0], [-4, 0.5, 0.25, 1, 0, 0]])
VIEW_INV = np.arange(16, dtype=np.float32).reshape(4, 4) * np.float32(0.5)
PROJ_INV = np.arange(16, dtype=np.float32)[::-1].reshape(4, 4) - np.float32(3.25)
W, H = 4, 2
TMAX_PER_RAY = np.float32([1.5, 2.5, 1e30])
STRUCTS = ("TraceArgs", "BvhTraceArgs", "TlasTraceArgs", "MultiHitArgs", "BvhMultiHitArgs", "TlasMultiHitArgs")


def base_of(a):
    """the TraceArgs of an argument structure, spelled per structure"""
    return {"TraceArgs": lambda: a, "BvhTraceArgs": lambda: a.base, "TlasTraceArgs": lambda: a.base, "MultiHitArgs": lambda: a.base,
            "BvhMultiHitArgs": lambda: a.m.base, "TlasMultiHitArgs": lambda: a.m.base}[type(a).__name__]()


def untouched_outputs(b):
    return not (b.t or b.prim or b.normal or b.shadowed or b.hits or b.num_hits or b.any_hit)


@pytest.mark.parametrize("name", STRUCTS)
def test_ray_batch_host_rays(vx, name):
    a = getattr(vx, name)()
    keep = []
    n = vx._ray_batch(base_of(a), RAYS.tolist(), None, 0.25, 77.5, TMAX_PER_RAY.tolist(), keep)
    b = base_of(a)
    assert n == 3 and b.num_rays == 3
    held = {k.ctypes.data: k for k in keep}
    r, tm = held[b.rays], held[b.tmax_per_ray]
    assert r.dtype == np.float32 and r.shape == (3, 6) and r.flags.c_contiguous and np.array_equal(r, RAYS)
    assert tm.dtype == np.float32 and tm.flags.c_contiguous and np.array_equal(tm, TMAX_PER_RAY)
    assert b.tmin == 0.25 and b.tmax == 77.5
    assert not b.view_inverse and not b.proj_inverse and b.width == 0 and b.height == 0
    assert untouched_outputs(b)


@pytest.mark.parametrize("name", STRUCTS)
def test_ray_batch_raw_pointer(vx, name):
    a = getattr(vx, name)()
    keep = []
    n = vx._ray_batch(base_of(a), (0x7F0000001000, 3), None, 0.001, 10000.0, None, keep)
    b = base_of(a)
    assert n == 3 and b.rays == 0x7F0000001000 and b.num_rays == 3 and not keep
    assert b.tmin == np.float32(0.001) and b.tmax == 10000.0 and not b.tmax_per_ray
    assert not b.view_inverse and not b.proj_inverse and b.width == 0 and b.height == 0
    assert untouched_outputs(b)
    vx._ray_batch(base_of(a), (None, 0), None, 0.0, 1.0, None, keep)     # no rays: a null pointer and a count of 0
    assert not base_of(a).rays and base_of(a).num_rays == 0


@pytest.mark.parametrize("name", STRUCTS)
def test_ray_batch_camera(vx, name):
    a = getattr(vx, name)()
    keep = []
    n = vx._ray_batch(base_of(a), None, (VIEW_INV, PROJ_INV, W, H), 0.5, 9.0, TMAX_PER_RAY, keep)
    b = base_of(a)
    assert n == 8 and b.width == 4 and b.height == 2
    assert not b.rays and b.num_rays == 0
    assert [b.view_inverse[i] for i in range(16)] == [float(x) for x in VIEW_INV.reshape(16)]
    assert [b.proj_inverse[i] for i in range(16)] == [float(x) for x in PROJ_INV.reshape(16)]
    assert b.tmin == 0.5 and b.tmax == 9.0
    assert len(keep) == 3 and keep[2].ctypes.data == b.tmax_per_ray and np.array_equal(keep[2], TMAX_PER_RAY)
    assert untouched_outputs(b)


FIRST_HIT = {"t": ((), np.float32), "prim": ((), np.uint32), "normal": ((3,), np.float32), "shadowed": ((), np.uint8),
             "bary": ((2,), np.float32), "instance": ((), np.uint32)}
MULTI_HIT = {"t": ((5,), np.float32), "prim": ((5,), np.uint32), "bary": ((5, 2), np.float32), "instance": ((5,), np.uint32),
             "count": ((), np.uint32)}
# what each structure has beside t and prim, and where the pointer of each output lies
HAS = {"TraceArgs": ("normal", "shadowed"), "BvhTraceArgs": ("normal", "shadowed", "bary"),
       "TlasTraceArgs": ("normal", "shadowed", "bary", "instance"), "MultiHitArgs": ("count",), "BvhMultiHitArgs": ("count", "bary"),
       "TlasMultiHitArgs": ("count", "bary", "instance")}


def pointer_of(a, name):
    if name in ("bary", "instance"):
        return getattr(a, name)
    if name == "count":
        return a.count if type(a).__name__ == "MultiHitArgs" else a.m.count
    return getattr(base_of(a), name)


@pytest.mark.parametrize("name", STRUCTS)
def test_outputs_shapes_and_dtypes(vx, name):
    multi = "Multi" in name
    doc = MULTI_HIT if multi else FIRST_HIT
    table = vx._multi_hit(5) if multi else vx._FIRST_HIT
    assert set(table) == set(doc)
    names = ("t", "prim") + HAS[name]
    a = getattr(vx, name)()
    out = vx._outputs(a, names, 7, table)
    assert set(out) == set(names)
    for k in names:
        assert out[k].shape == (7,) + doc[k][0] and out[k].dtype == doc[k][1] and out[k].flags.c_contiguous and not out[k].any(), k
        assert pointer_of(a, k) == out[k].ctypes.data, k
    a = getattr(vx, name)()
    assert list(vx._outputs(a, ("prim",), 2, table)) == ["prim"] and not base_of(a).t      # only what was asked for
    assert vx._outputs(getattr(vx, name)(), (), 2, table) == {}


def test_outputs_refuse_what_the_structure_lacks(vx):
    for a, table in ((vx.TraceArgs(), vx._FIRST_HIT), (vx.MultiHitArgs(), vx._multi_hit(2))):
        with pytest.raises(ValueError) as e:
            vx._outputs(a, ("t", "bary"), 3, table)
        assert str(e.value) == "bary is an output of the triangle BVH only"
    for a, table in ((vx.BvhTraceArgs(), vx._FIRST_HIT), (vx.BvhMultiHitArgs(), vx._multi_hit(2))):
        with pytest.raises(ValueError) as e:
            vx._outputs(a, ("t", "instance"), 3, table)
        assert str(e.value) == "instance is an output of the TLAS only"


def test_public_signatures(vx):
    import inspect
    sig = inspect.signature(vx.Tlas.trace_ex).parameters
    assert sig["want"].default == ("t", "instance", "prim", "bary", "normal")
    assert "camera" not in inspect.signature(vx.Tlas.trace_device).parameters
    for cls in (vx.Grid, vx.Octree, vx.Bvh):
        assert inspect.signature(cls.trace_ex).parameters["want"].default == ("t", "prim")
        assert inspect.signature(cls.trace_multi).parameters["want"].default == ("t", "prim", "count")
    assert inspect.signature(vx.Tlas.trace_multi).parameters["want"].default == ("t", "instance", "prim", "count")


RAY_ENTRIES = (("vx_trace_ex", "TraceArgs"), ("vx_trace_ex_device", "TraceArgs"), ("vx_octree_trace_ex", "TraceArgs"),
               ("vx_octree_trace_ex_device", "TraceArgs"), ("vx_bvh_trace_ex", "BvhTraceArgs"), ("vx_bvh_trace_ex_device", "BvhTraceArgs"),
               ("vx_tlas_trace_ex", "TlasTraceArgs"), ("vx_tlas_trace_ex_device", "TlasTraceArgs"),
               ("vx_trace_multi", "MultiHitArgs"), ("vx_trace_multi_device", "MultiHitArgs"), ("vx_octree_trace_multi", "MultiHitArgs"),
               ("vx_octree_trace_multi_device", "MultiHitArgs"), ("vx_bvh_trace_multi", "BvhMultiHitArgs"),
               ("vx_bvh_trace_multi_device", "BvhMultiHitArgs"), ("vx_tlas_trace_multi", "TlasMultiHitArgs"),
               ("vx_tlas_trace_multi_device", "TlasMultiHitArgs"))


def null_handle_refused(vx, status):
    assert status == INVALID_ARG
    assert vx.lib().vx_last_error() == b"null argument"


@pytest.mark.parametrize("fn,struct", RAY_ENTRIES)
def test_ray_entry_null_handle(vx, fn, struct):
    a = getattr(vx, struct)()
    t = np.full(3, 7.0, np.float32)
    vx._ray_batch(base_of(a), RAYS, None, 0.001, 10000.0, None, [])
    base_of(a).t = t.ctypes.data
    if "multi" in fn:
        (a if struct == "MultiHitArgs" else a.m).max_hits = 1
    null_handle_refused(vx, getattr(vx.lib(), fn)(None, C.byref(a)))
    null_handle_refused(vx, getattr(vx.lib(), fn)(None, None))
    assert (t == 7.0).all()


def test_field_entry_null_handle(vx):
    L = vx.lib()
    out = np.full(8, 7, np.uint32)
    val = np.zeros(8, np.uint32)
    o, v = out.ctypes.data, val.ctypes.data
    for fn in (L.vx_grid_distance_sq, L.vx_grid_distance_sq_device, L.vx_grid_nearest, L.vx_grid_nearest_device):
        null_handle_refused(vx, fn(None, 0, o, 8))
    for fn in (L.vx_grid_sdf, L.vx_grid_sdf_device):
        null_handle_refused(vx, fn(None, o, 8))
    for fn in (L.vx_grid_nearest_gather, L.vx_grid_nearest_gather_device):
        null_handle_refused(vx, fn(None, 0, v, 8, 0, o, 8))
    for fn in (L.vx_grid_morph_mask, L.vx_grid_morph_device):
        null_handle_refused(vx, fn(None, vx.MORPH_DILATE, 1, o, 8))
    assert (out == 7).all()
