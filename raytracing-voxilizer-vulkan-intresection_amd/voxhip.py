"""ctypes plumbing over libvoxhip.so (the C ABI of include/voxhip.h) for tests, bench.py and __graft_entry__.

This is NOT a second implementation: every call lands in the HIP library; if the library is missing the import
fails loudly.  Nothing here imports or falls back to oracle/.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvoxhip.so")

VX_OK = 0
GRID_BOOL, GRID_AABBSTRUCT, GRID_VEC = 0, 1, 2
VOXELIZE_MATERIALS = 1
VOXELIZE_LIST_ASYNC = 2
VOXELIZE_SOLID = 4
DISTANCE_INSIDE = 1
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3   # VX_MORPH_*
CONNECT_6, CONNECT_26 = 6, 26
STATUS_NAMES = {0: "VX_OK", 1: "VX_ERR_INVALID_ARG", 2: "VX_ERR_PATH", 3: "VX_ERR_PARSE", 4: "VX_ERR_OUT_OF_BOUNDS",
                5: "VX_ERR_MORTON_BITS", 6: "VX_ERR_NO_DEVICE", 7: "VX_ERR_HIP", 8: "VX_ERR_CAPACITY", 9: "VX_ERR_UNSUPPORTED"}

AABB = np.dtype([("mn", np.float32, 3), ("mx", np.float32, 3)])
NODE = np.dtype([("children", np.uint32, 8), ("start", np.uint32), ("count", np.uint32)])
HIT = np.dtype([("ray", np.uint32), ("prim", np.uint32), ("t", np.float32)])
COMPONENT = np.dtype([("cells", np.uint64), ("min", np.uint32, 3), ("max", np.uint32, 3)])  # vx_component, 32 B
BVH_NODE = np.dtype([("mn", np.float32, 3), ("a", np.uint32), ("mx", np.float32, 3), ("b", np.uint32)])   # vx_bvh_node
BVH_LEAF = 0x80000000
MATERIAL = np.dtype([("ambient", np.float32, 3), ("diffuse", np.float32, 3), ("specular", np.float32, 3), ("transmittance", np.float32, 3),
                     ("emission", np.float32, 3), ("shininess", np.float32), ("ior", np.float32), ("dissolve", np.float32),
                     ("illum", np.int32), ("texture_id", np.int32)])


def _levels(a):
    """An argument structure and the structures it leads with, outermost first: TlasMultiHitArgs -> [a, a.m, a.m.base], BvhTraceArgs ->
    [a, a.base], TraceArgs -> [a].  The last one is always the TraceArgs."""
    lv = [a]
    for f in ("m", "base"):
        if hasattr(lv[-1], f):
            lv.append(getattr(lv[-1], f))
    return lv


def _ray_batch(base, rays, camera, tmin, tmax, tmax_per_ray, keep):
    """Fills the ray batch of a TraceArgs (the .base of any of the six argument structures) and returns the number of rays.  rays: host
    rays, anything that becomes contiguous float32 (n, 6), or a raw (pointer, n); None: camera = (view_inv, proj_inv, width, height).
    tmax_per_ray: a host array or None.  What the structure then points at goes into `keep`, which the caller holds over the call."""
    if rays is None:
        vi, pi, w, h = camera
        cvi, cpi = [(C.c_float * 16)(*[float(x) for x in np.asarray(m).reshape(16)]) for m in (vi, pi)]
        keep += [cvi, cpi]
        base.view_inverse, base.proj_inverse, base.width, base.height, n = cvi, cpi, w, h, w * h
    elif isinstance(rays, tuple) and len(rays) == 2 and not hasattr(rays[0], "__len__"):
        base.rays, base.num_rays = rays
        n = rays[1]
    else:
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        keep.append(r)
        base.rays, base.num_rays, n = r.ctypes.data, r.shape[0], r.shape[0]
    base.tmin, base.tmax = np.float32(tmin), np.float32(tmax)
    if tmax_per_ray is not None:
        tm = np.ascontiguousarray(tmax_per_ray, dtype=np.float32)
        keep.append(tm)
        base.tmax_per_ray = tm.ctypes.data
    return n


# the outputs of the first-hit queries: name -> (shape behind the ray index, dtype)
_FIRST_HIT = {"t": ((), np.float32), "prim": ((), np.uint32), "normal": ((3,), np.float32), "shadowed": ((), np.uint8),
              "bary": ((2,), np.float32), "instance": ((), np.uint32)}
_NOT_HERE = {"bary": "bary is an output of the triangle BVH only", "instance": "instance is an output of the TLAS only"}


def _multi_hit(k):
    """the outputs of the multi-hit queries at max_hits = k, as _FIRST_HIT"""
    return {"t": ((k,), np.float32), "prim": ((k,), np.uint32), "bary": ((k, 2), np.float32), "instance": ((k,), np.uint32),
            "count": ((), np.uint32)}


def _outputs(a, want, n, table):
    """Allocates the arrays of `table` that `want` names, (n,) + shape each and zeroed, and points the field of that name at each: the
    field of `a` or of a structure it leads with (_levels).  A name the structure has no field for is a ValueError.  -> dict name -> array"""
    out = {}
    for name, (shape, dtype) in table.items():
        if name not in want:
            continue
        owner = [s for s in _levels(a) if hasattr(s, name)]
        if not owner:
            raise ValueError(_NOT_HERE[name])
        out[name] = np.zeros((n,) + shape, dtype)
        setattr(owner[0], name, out[name].ctypes.data)
    return out


def _set_pointers(a, ptrs):
    """the device variants' arrays: field name -> raw device pointer, each into the structure of _levels(a) that has the field"""
    for name, p in ptrs.items():
        setattr([s for s in _levels(a) if hasattr(s, name)][0], name, p)


def _trace_ex(fn, h, a, rays, camera, tmin, tmax, tmax_per_ray, any_hit, want):
    """vx_*_trace_ex (a = the handle's TraceArgs / BvhTraceArgs / TlasTraceArgs) on host arrays -> dict of the requested outputs (t, prim,
    normal, shadowed; bary for the BVH and the TLAS; instance for the TLAS)."""
    base, keep = _levels(a)[-1], []
    n = _ray_batch(base, rays, camera, tmin, tmax, tmax_per_ray, keep)
    base.any_hit = 1 if any_hit else 0
    out = _outputs(a, want, n, _FIRST_HIT)
    _check(fn(h, C.byref(a)))
    return out


def _trace_ex_device(fn, h, a, rays_ptr, nrays, camera, tmin, tmax, any_hit, **ptrs):
    """vx_*_trace_ex_device on raw device pointers (ptrs: field name -> pointer), asynchronous on the handle's stream; camera =
    (view_inv, proj_inv, width, height) in place of rays_ptr / nrays."""
    base, keep = _levels(a)[-1], []
    _ray_batch(base, (rays_ptr, nrays) if camera is None else None, camera, tmin, tmax, None, keep)
    base.any_hit = 1 if any_hit else 0
    _set_pointers(a, ptrs)
    _check(fn(h, C.byref(a)))


def _trace_multi(fn, h, a, cursor, rays, camera, max_hits, tmin, tmax, tmax_per_ray, after, want):
    """vx_*_trace_multi (a = the handle's MultiHitArgs / BvhMultiHitArgs / TlasMultiHitArgs, cursor = the arrays of its cursor: 2, or 3 for
    the TLAS) on host arrays -> dict of the requested outputs: t (n, K) float32, prim and instance (n, K) uint32, bary (n, K, 2) float32,
    padded with -1 / 0xFFFFFFFF / (0, 0); count (n,) uint32."""
    m, keep = _levels(a)[-2], []
    n = _ray_batch(m.base, rays, camera, tmin, tmax, tmax_per_ray, keep)
    m.max_hits = int(max_hits)
    if after is not None:
        # (the grid and the octree have one text for both mistakes, the mesh structures one each)
        texts = ("after = (after_t, after_prim), one entry per ray each",) * 2 if m is a else (
            "after = (after_t, after_instance, after_prim)" if cursor == 3 else "after = (after_t, after_prim)",
            "the cursor has one entry per ray in each of its arrays")
        if len(after) != cursor:
            raise ValueError(texts[0])
        cur = [np.ascontiguousarray(after[0], dtype=np.float32)] + [np.ascontiguousarray(x, dtype=np.uint32) for x in after[1:]]
        if any(c.shape != (n,) for c in cur):
            raise ValueError(texts[1])
        keep += cur
        m.after_t, m.after_prim = cur[0].ctypes.data, cur[-1].ctypes.data
        if cursor == 3:
            a.after_instance = cur[1].ctypes.data
    out = _outputs(a, want, n, _multi_hit(max(int(max_hits), 0)))
    _check(fn(h, C.byref(a)))
    return out


def _trace_multi_device(fn, h, a, rays_ptr, nrays, camera, max_hits, tmin, tmax, **ptrs):
    """vx_*_trace_multi_device on raw device pointers (ptrs: field name -> pointer), asynchronous on the handle's stream; camera =
    (view_inv, proj_inv, width, height) in place of rays_ptr / nrays."""
    m, keep = _levels(a)[-2], []
    _ray_batch(m.base, (rays_ptr, nrays) if camera is None else None, camera, tmin, tmax, None, keep)
    m.max_hits = int(max_hits)
    _set_pointers(a, ptrs)
    _check(fn(h, C.byref(a)))


class GridDesc(C.Structure):
    _fields_ = [("dim", C.c_uint64 * 3), ("voxel_size", C.c_float), ("origin", C.c_float * 3), ("bbox_min", C.c_float * 3),
                ("bbox_max", C.c_float * 3), ("bbox_center", C.c_float * 3), ("num_words", C.c_uint64), ("set_calls", C.c_uint64),
                ("occupied", C.c_uint64), ("triangles", C.c_uint64), ("kind", C.c_int32), ("device", C.c_int32)]


class VoxelizeOpts(C.Structure):
    _fields_ = [("sat_variant", C.c_int32), ("flags", C.c_int32), ("word_begin", C.c_uint64), ("word_end", C.c_uint64),
                ("tri_begin", C.c_uint64), ("tri_end", C.c_uint64), ("stream", C.c_void_p), ("shard_rank", C.c_int32), ("shard_world", C.c_int32)]


class Smooth(C.Structure):
    """vx_smooth: iterations x (a step with lambda, then a step with mu when mu != 0)"""
    _fields_ = [("iterations", C.c_uint32), ("lam", C.c_float), ("mu", C.c_float)]


class ScanArgs(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("nscans", C.c_uint32), ("sizes", C.c_void_p), ("paths", C.c_void_p), ("inp", C.c_void_p), ("out", C.c_void_p),
                ("totals", C.c_void_p), ("taken", C.c_void_p), ("clean", C.c_void_p), ("sel", C.c_void_p), ("group16", C.c_void_p),
                ("sel_cap", C.c_uint64), ("group16_cap", C.c_uint64), ("in_offset", C.c_uint64), ("out_offset", C.c_uint64),
                ("total_tag", C.c_uint64), ("gen_start", C.c_uint32), ("pad", C.c_uint32)]


class FieldDesc(C.Structure):
    _fields_ = [("dim", C.c_uint64 * 3), ("voxel_size", C.c_float), ("origin", C.c_float * 3), ("state", C.c_uint32), ("bytes", C.c_uint64)]


class FieldSampleArgs(C.Structure):
    _fields_ = [("points", C.c_void_p), ("num_points", C.c_uint64), ("value", C.c_void_p), ("gradient", C.c_void_p), ("occupied", C.c_void_p)]


class FieldTraceArgs(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("num_rays", C.c_uint64), ("tmin", C.c_float), ("tmax", C.c_float), ("tmax_per_ray", C.c_void_p),
                ("radius", C.c_float), ("radius_per_ray", C.c_void_p), ("step_scale", C.c_float), ("hit_eps", C.c_float),
                ("max_steps", C.c_uint32), ("t", C.c_void_p), ("clearance", C.c_void_p), ("steps", C.c_void_p), ("status", C.c_void_p)]


class FieldPoseArgs(C.Structure):
    _fields_ = [("points", C.c_void_p), ("num_points", C.c_uint64), ("radii", C.c_void_p), ("transforms", C.c_void_p), ("num_poses", C.c_uint64),
                ("margin", C.c_float), ("clearance", C.c_void_p), ("point", C.c_void_p), ("count", C.c_void_p), ("position", C.c_void_p),
                ("gradient", C.c_void_p)]


class TraceArgs(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("view_inverse", C.POINTER(C.c_float)), ("proj_inverse", C.POINTER(C.c_float)), ("width", C.c_uint32),
                ("height", C.c_uint32), ("num_rays", C.c_uint64), ("tmin", C.c_float), ("tmax", C.c_float), ("tmax_per_ray", C.c_void_p),
                ("any_hit", C.c_int32), ("reserved", C.c_int32), ("t", C.c_void_p), ("prim", C.c_void_p), ("normal", C.c_void_p),
                ("shadowed", C.c_void_p), ("hits", C.c_void_p), ("num_hits", C.c_void_p)]


class MultiHitArgs(C.Structure):
    _fields_ = [("base", TraceArgs), ("max_hits", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_void_p), ("after_t", C.c_void_p),
                ("after_prim", C.c_void_p)]


MULTIHIT_MAX = 32   # VX_MULTIHIT_MAX


class BvhTraceArgs(C.Structure):
    _fields_ = [("base", TraceArgs), ("bary", C.c_void_p)]


class TlasTraceArgs(C.Structure):
    _fields_ = [("base", TraceArgs), ("bary", C.c_void_p), ("instance", C.c_void_p)]


class BvhMultiHitArgs(C.Structure):
    _fields_ = [("m", MultiHitArgs), ("bary", C.c_void_p)]


class TlasMultiHitArgs(C.Structure):
    _fields_ = [("m", MultiHitArgs), ("bary", C.c_void_p), ("instance", C.c_void_p), ("after_instance", C.c_void_p)]


# vx_instance: object-to-world (row-major 3x4), BLAS index, mask (0 = never hit)
INSTANCE = np.dtype([("transform", np.float32, (12,)), ("blas", np.uint32), ("mask", np.uint32)])


RENDER_ATTRIBUTES = 1   # VX_RENDER_ATTRIBUTES


class RenderLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("intensity", C.c_float), ("type", C.c_int32)]


class RenderDesc(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("octree", C.c_void_p), ("bvh", C.c_void_p), ("mesh", C.c_void_p), ("stream", C.c_void_p)]


class RenderTlasDesc(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("octree", C.c_void_p), ("tlas", C.c_void_p), ("meshes", C.c_void_p), ("stream", C.c_void_p)]


class RenderArgs(C.Structure):
    _fields_ = [("view_inverse", C.POINTER(C.c_float)), ("proj_inverse", C.POINTER(C.c_float)), ("width", C.c_uint32), ("height", C.c_uint32),
                ("light", C.POINTER(RenderLight)), ("rgba", C.c_void_p), ("kind", C.c_void_p), ("shadowed", C.c_void_p)]


class VxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), msg))
        self.status = status
        self.message = msg


# every symbol include/voxhip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "vx_last_error", "vx_status_string", "vx_device_count", "vx_set_device", "vx_release_cached_memory",
    "vx_mesh_load_obj", "vx_mesh_from_arrays", "vx_mesh_from_device", "vx_mesh_num_vertices", "vx_mesh_num_triangles",
    "vx_mesh_host_vertices", "vx_mesh_host_indices", "vx_mesh_num_materials", "vx_mesh_materials", "vx_mesh_host_material_ids",
    "vx_mesh_set_materials", "vx_mesh_free",
    "vx_mesh_host_corner_normals", "vx_mesh_host_corner_uvs", "vx_mesh_set_attributes", "vx_mesh_num_textures", "vx_mesh_texture_name",
    "vx_mesh_host_texture", "vx_mesh_host_material_textures", "vx_mesh_set_material_textures", "vx_mesh_set_texture", "vx_mesh_load_textures",
    "vx_voxelize", "vx_voxelize_into", "vx_voxelize_multi",
    "vx_grid_create", "vx_grid_describe", "vx_grid_set_voxel", "vx_grid_test_voxel", "vx_grid_coords", "vx_grid_bytes",
    "vx_grid_bitmask", "vx_grid_bitmask_device", "vx_grid_bitmask_device_mut", "vx_grid_refresh", "vx_grid_fill_interior", "vx_grid_interior", "vx_grid_fill_rounds",
    "vx_grid_distance_sq_device", "vx_grid_distance_sq", "vx_grid_sdf_device", "vx_grid_sdf",
    "vx_grid_nearest_device", "vx_grid_nearest", "vx_grid_nearest_gather_device", "vx_grid_nearest_gather",
    "vx_field_create", "vx_field_update", "vx_field_describe", "vx_field_values_device", "vx_field_free",
    "vx_field_sample_device", "vx_field_sample", "vx_field_sphere_trace_device", "vx_field_sphere_trace",
    "vx_field_poses_device", "vx_field_poses",
    "vx_grid_morph_device", "vx_grid_morph_mask", "vx_grid_morph", "vx_grid_seal", "vx_morph_bit_radius",
    "vx_grid_surface_device", "vx_grid_surface", "vx_grid_surface_mesh",
    "vx_grid_surface_smooth_device", "vx_grid_surface_smooth", "vx_grid_surface_smooth_mesh",
    "vx_grid_components_device", "vx_grid_components", "vx_grid_component_stats", "vx_grid_aabbs",
    "vx_grid_aabbs_device", "vx_grid_bind_aabbs_device", "vx_grid_list_wait", "vx_grid_aabbs_device_async", "vx_grid_materials", "vx_grid_material_ids", "vx_grid_material_ids_device", "vx_grid_material_first_use",
    "vx_grid_finish_materials", "vx_multi_create", "vx_multi_voxelize", "vx_multi_grid", "vx_multi_release_grid", "vx_multi_free", "vx_sort_u64", "vx_scan_u32", "vx_grid_free",
    "vx_octree_build", "vx_octree_num_items", "vx_octree_num_nodes", "vx_octree_bytes", "vx_octree_items", "vx_octree_nodes",
    "vx_octree_root_bounds", "vx_octree_aabbs", "vx_octree_aabbs_device", "vx_octree_free",
    "vx_trace", "vx_trace_device", "vx_trace_primary_device", "vx_trace_ex", "vx_trace_ex_device",
    "vx_trace_multi", "vx_trace_multi_device",
    "vx_octree_trace", "vx_octree_trace_ex", "vx_octree_trace_ex_device", "vx_octree_trace_multi", "vx_octree_trace_multi_device",
    "vx_bvh_build", "vx_bvh_build_into", "vx_bvh_num_triangles", "vx_bvh_num_nodes", "vx_bvh_bytes", "vx_bvh_height", "vx_bvh_num_ill_conditioned", "vx_bvh_root_bounds",
    "vx_bvh_nodes", "vx_bvh_leaf_triangles", "vx_bvh_nodes_device", "vx_bvh_trace_ex_device", "vx_bvh_trace_ex", "vx_bvh_trace",
    "vx_bvh_trace_multi", "vx_bvh_trace_multi_device", "vx_bvh_free",
    "vx_tlas_build", "vx_tlas_update", "vx_tlas_update_device", "vx_tlas_num_instances", "vx_tlas_num_nodes", "vx_tlas_height", "vx_tlas_bytes",
    "vx_tlas_world_to_object", "vx_tlas_nodes", "vx_tlas_trace_ex_device", "vx_tlas_trace_ex", "vx_tlas_trace",
    "vx_tlas_trace_multi", "vx_tlas_trace_multi_device", "vx_tlas_free",
    "vx_render_create", "vx_render_create_tlas", "vx_render_refresh", "vx_render_set_shading", "vx_render_frame_device", "vx_render_frame", "vx_render_free",
    "vx_profile_enable", "vx_profile_select", "vx_profile_reset", "vx_profile_read", "vx_device_allocations", "vx_device_live_blocks",
    "vx_pool_poison", "vx_pool_poisoned_blocks",
    "vx_shard_words", "vx_shard_range",
]

_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's); if
    libvoxhip.so pulled in the system copy first, a later `import torch` would load a second runtime that sees no GPU.
    When torch is installed (tests, bench.py: device memory, streams, torch.distributed), bind to ITS runtime by loading
    it first; plain C/C++ users of libvoxhip.so get the system ROCm runtime via the library's RUNPATH."""
    if os.environ.get("VOXHIP_SYSTEM_HIP_RUNTIME") == "1":
        return
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libvoxhip.so is not built (%s): run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
    _preload_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, u64p, fp, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.vx_last_error.restype = C.c_char_p
    L.vx_status_string.restype = C.c_char_p
    L.vx_status_string.argtypes = [C.c_int]
    L.vx_device_count.restype = C.c_int
    L.vx_set_device.argtypes = [C.c_int]
    L.vx_mesh_load_obj.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.vx_mesh_from_arrays.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
    L.vx_mesh_from_device.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
    L.vx_mesh_num_vertices.argtypes = [vp]
    L.vx_mesh_num_vertices.restype = C.c_size_t
    L.vx_mesh_num_triangles.argtypes = [vp]
    L.vx_mesh_num_triangles.restype = C.c_size_t
    L.vx_mesh_host_vertices.argtypes = [vp]
    L.vx_mesh_host_vertices.restype = vp
    L.vx_mesh_host_indices.argtypes = [vp]
    L.vx_mesh_host_indices.restype = vp
    L.vx_mesh_num_materials.argtypes = [vp]
    L.vx_mesh_num_materials.restype = C.c_size_t
    L.vx_mesh_materials.argtypes = [vp, vp, C.c_size_t]
    L.vx_mesh_host_material_ids.argtypes = [vp]
    L.vx_mesh_host_material_ids.restype = vp
    L.vx_mesh_set_materials.argtypes = [vp, vp, C.c_size_t, vp]
    L.vx_mesh_free.argtypes = [vp]
    L.vx_mesh_free.restype = None
    for _f in ("vx_mesh_host_corner_normals", "vx_mesh_host_corner_uvs", "vx_mesh_host_material_textures"):
        getattr(L, _f).argtypes = [vp]
        getattr(L, _f).restype = vp
    L.vx_mesh_set_attributes.argtypes = [vp, vp, vp]
    L.vx_mesh_num_textures.argtypes = [vp]
    L.vx_mesh_num_textures.restype = C.c_size_t
    L.vx_mesh_texture_name.argtypes = [vp, C.c_size_t]
    L.vx_mesh_texture_name.restype = C.c_char_p
    L.vx_mesh_host_texture.argtypes = [vp, C.c_size_t, u32p, u32p]
    L.vx_mesh_host_texture.restype = vp
    L.vx_mesh_set_material_textures.argtypes = [vp, vp, C.c_size_t]
    L.vx_mesh_set_texture.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint32, vp]
    L.vx_mesh_load_textures.argtypes = [vp]
    L.vx_voxelize.argtypes = [vp, C.c_float, C.c_int, C.POINTER(VoxelizeOpts), C.POINTER(vp)]
    L.vx_voxelize_into.argtypes = [vp, C.c_float, C.POINTER(VoxelizeOpts), vp]
    L.vx_voxelize_multi.argtypes = [vp, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(vp)]
    L.vx_sort_u64.argtypes = [vp, C.c_uint64, C.c_int]
    L.vx_scan_u32.argtypes = [C.POINTER(ScanArgs)]
    L.vx_multi_create.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(vp)]
    L.vx_multi_voxelize.argtypes = [vp, C.c_float, vp, C.c_int]
    L.vx_multi_grid.argtypes = [vp, C.c_int]
    L.vx_multi_grid.restype = vp
    L.vx_multi_release_grid.argtypes = [vp, C.c_int]
    L.vx_multi_release_grid.restype = vp
    L.vx_multi_free.argtypes = [vp]
    L.vx_multi_free.restype = None
    L.vx_grid_material_first_use.argtypes = [vp, C.POINTER(C.c_int64), C.c_uint64, C.POINTER(C.c_uint64)]
    L.vx_grid_finish_materials.argtypes = [vp, C.POINTER(C.c_int64), C.c_uint64]
    L.vx_grid_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, fp, vp, C.POINTER(vp)]
    L.vx_grid_describe.argtypes = [vp, C.POINTER(GridDesc)]
    L.vx_grid_set_voxel.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.vx_grid_test_voxel.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]
    L.vx_grid_coords.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, fp]
    L.vx_grid_bytes.argtypes = [vp]
    L.vx_grid_bytes.restype = C.c_uint64
    L.vx_grid_bitmask.argtypes = [vp, vp, C.c_uint64]
    L.vx_grid_bitmask_device.argtypes = [vp]
    L.vx_grid_bitmask_device.restype = vp
    L.vx_grid_bitmask_device_mut.argtypes = [vp]
    L.vx_grid_bitmask_device_mut.restype = vp
    L.vx_grid_refresh.argtypes = [vp]
    L.vx_grid_fill_interior.argtypes = [vp]
    L.vx_grid_interior.argtypes = [vp, u64p]
    L.vx_grid_fill_rounds.argtypes = [vp]
    L.vx_grid_fill_rounds.restype = C.c_uint32
    L.vx_grid_distance_sq_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_distance_sq.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_sdf_device.argtypes = [vp, vp, C.c_uint64]
    L.vx_grid_sdf.argtypes = [vp, vp, C.c_uint64]
    L.vx_field_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.vx_field_update.argtypes = [vp, vp]
    L.vx_field_describe.argtypes = [vp, C.POINTER(FieldDesc)]
    L.vx_field_values_device.argtypes = [vp]
    L.vx_field_values_device.restype = vp
    L.vx_field_free.argtypes = [vp]
    L.vx_field_free.restype = None
    L.vx_field_sample_device.argtypes = [vp, C.POINTER(FieldSampleArgs)]
    L.vx_field_sample.argtypes = [vp, C.POINTER(FieldSampleArgs)]
    L.vx_field_sphere_trace_device.argtypes = [vp, C.POINTER(FieldTraceArgs)]
    L.vx_field_sphere_trace.argtypes = [vp, C.POINTER(FieldTraceArgs)]
    L.vx_field_poses_device.argtypes = [vp, C.POINTER(FieldPoseArgs)]
    L.vx_field_poses.argtypes = [vp, C.POINTER(FieldPoseArgs)]
    L.vx_grid_nearest_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_nearest.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_nearest_gather_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_nearest_gather.argtypes = [vp, C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_morph_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_morph_mask.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64]
    L.vx_grid_morph.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.vx_grid_seal.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.vx_morph_bit_radius.argtypes = []
    L.vx_morph_bit_radius.restype = C.c_uint32
    L.vx_grid_surface_device.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, u64p, u64p]
    L.vx_grid_surface.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, u64p, u64p]
    L.vx_grid_surface_mesh.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.vx_grid_surface_smooth_device.argtypes = [vp, C.POINTER(Smooth), vp, C.c_uint64, vp, C.c_uint64, vp, vp, u64p, u64p]
    L.vx_grid_surface_smooth.argtypes = [vp, C.POINTER(Smooth), vp, C.c_uint64, vp, C.c_uint64, vp, vp, u64p, u64p]
    L.vx_grid_surface_smooth_mesh.argtypes = [vp, C.POINTER(Smooth), C.c_int, C.c_int, C.POINTER(vp)]
    L.vx_grid_components_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
    L.vx_grid_components.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    L.vx_grid_component_stats.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    L.vx_grid_aabbs.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_grid_aabbs_device.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_grid_bind_aabbs_device.argtypes = [vp, vp, C.c_uint64]
    L.vx_grid_list_wait.argtypes = [vp]
    L.vx_grid_aabbs_device_async.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_grid_materials.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_grid_material_ids.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_grid_material_ids_device.argtypes = [vp]
    L.vx_grid_material_ids_device.restype = vp
    L.vx_grid_free.argtypes = [vp]
    L.vx_grid_free.restype = None
    L.vx_octree_build.argtypes = [vp, C.c_float, C.c_uint64, vp, C.POINTER(vp)]
    for n in ("vx_octree_num_items", "vx_octree_num_nodes", "vx_octree_bytes"):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = C.c_uint64
    L.vx_octree_items.argtypes = [vp, vp, C.c_uint64]
    L.vx_octree_nodes.argtypes = [vp, vp, C.c_uint64]
    L.vx_octree_root_bounds.argtypes = [vp, fp, fp]
    L.vx_octree_aabbs.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_octree_aabbs_device.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_octree_free.argtypes = [vp]
    L.vx_octree_free.restype = None
    L.vx_trace.argtypes = [vp, vp, C.c_uint64, C.c_float, C.c_float, vp, vp, u64p]
    L.vx_trace_device.argtypes = [vp, vp, C.c_uint64, C.c_float, C.c_float, vp, vp, vp, vp]
    L.vx_trace_primary_device.argtypes = [vp, fp, fp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp, vp]
    L.vx_profile_enable.argtypes = [C.c_int]
    L.vx_profile_select.argtypes = [C.c_char_p]
    L.vx_profile_read.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), u64p]
    L.vx_trace_ex.argtypes = [vp, C.POINTER(TraceArgs)]
    L.vx_trace_ex_device.argtypes = [vp, C.POINTER(TraceArgs)]
    L.vx_trace_multi.argtypes = [vp, C.POINTER(MultiHitArgs)]
    L.vx_trace_multi_device.argtypes = [vp, C.POINTER(MultiHitArgs)]
    L.vx_octree_trace.argtypes = [vp, vp, C.c_uint64, C.c_float, C.c_float, vp, vp, u64p]
    L.vx_octree_trace_ex.argtypes = [vp, C.POINTER(TraceArgs)]
    L.vx_octree_trace_ex_device.argtypes = [vp, C.POINTER(TraceArgs)]
    L.vx_octree_trace_multi.argtypes = [vp, C.POINTER(MultiHitArgs)]
    L.vx_octree_trace_multi_device.argtypes = [vp, C.POINTER(MultiHitArgs)]
    L.vx_bvh_build.argtypes = [vp, C.c_uint32, vp, C.POINTER(vp)]
    L.vx_bvh_build_into.argtypes = [vp, vp]
    for n in ("vx_bvh_num_triangles", "vx_bvh_num_nodes", "vx_bvh_bytes"):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = C.c_uint64
    L.vx_bvh_height.argtypes = [vp]
    L.vx_bvh_height.restype = C.c_uint32
    L.vx_bvh_num_ill_conditioned.argtypes = [vp]
    L.vx_bvh_num_ill_conditioned.restype = C.c_uint64
    L.vx_device_allocations.argtypes = []
    L.vx_device_allocations.restype = C.c_uint64
    L.vx_device_live_blocks.argtypes = []
    L.vx_device_live_blocks.restype = C.c_uint64
    L.vx_pool_poison.argtypes = [C.c_int, C.c_uint32]
    L.vx_pool_poisoned_blocks.argtypes = []
    L.vx_pool_poisoned_blocks.restype = C.c_uint64
    L.vx_bvh_root_bounds.argtypes = [vp, fp, fp]
    L.vx_bvh_nodes.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_bvh_leaf_triangles.argtypes = [vp, vp, C.c_uint64]
    L.vx_bvh_nodes_device.argtypes = [vp]
    L.vx_bvh_nodes_device.restype = vp
    L.vx_bvh_trace_ex.argtypes = [vp, C.POINTER(BvhTraceArgs)]
    L.vx_bvh_trace_ex_device.argtypes = [vp, C.POINTER(BvhTraceArgs)]
    L.vx_bvh_trace.argtypes = [vp, vp, C.c_uint64, C.c_float, C.c_float, vp, vp, u64p]
    L.vx_bvh_trace_multi.argtypes = [vp, C.POINTER(BvhMultiHitArgs)]
    L.vx_bvh_trace_multi_device.argtypes = [vp, C.POINTER(BvhMultiHitArgs)]
    L.vx_tlas_trace_multi.argtypes = [vp, C.POINTER(TlasMultiHitArgs)]
    L.vx_tlas_trace_multi_device.argtypes = [vp, C.POINTER(TlasMultiHitArgs)]
    L.vx_bvh_free.argtypes = [vp]
    L.vx_bvh_free.restype = None
    L.vx_tlas_build.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, C.POINTER(vp)]
    L.vx_tlas_update.argtypes = [vp, vp, C.c_uint64]
    L.vx_tlas_update_device.argtypes = [vp, vp, C.c_uint64]
    for _f in ("vx_tlas_num_instances", "vx_tlas_num_nodes", "vx_tlas_bytes"):
        getattr(L, _f).argtypes = [vp]
        getattr(L, _f).restype = C.c_uint64
    L.vx_tlas_height.argtypes = [vp]
    L.vx_tlas_height.restype = C.c_uint32
    L.vx_tlas_world_to_object.argtypes = [vp, vp, C.c_uint64]
    L.vx_tlas_nodes.argtypes = [vp, vp, C.c_uint64, u64p]
    L.vx_tlas_trace_ex.argtypes = [vp, C.POINTER(TlasTraceArgs)]
    L.vx_tlas_trace_ex_device.argtypes = [vp, C.POINTER(TlasTraceArgs)]
    L.vx_tlas_trace.argtypes = [vp, vp, C.c_uint64, C.c_float, C.c_float, vp, vp, vp, u64p]
    L.vx_tlas_free.argtypes = [vp]
    L.vx_tlas_free.restype = None
    L.vx_render_create_tlas.argtypes = [C.POINTER(RenderTlasDesc), C.POINTER(vp)]
    L.vx_render_create.argtypes = [C.POINTER(RenderDesc), C.POINTER(vp)]
    L.vx_render_refresh.argtypes = [vp]
    L.vx_render_set_shading.argtypes = [vp, C.c_uint32]
    L.vx_render_frame_device.argtypes = [vp, C.POINTER(RenderArgs)]
    L.vx_render_frame.argtypes = [vp, C.POINTER(RenderArgs)]
    L.vx_render_free.argtypes = [vp]
    L.vx_render_free.restype = None
    L.vx_shard_words.argtypes = [C.c_uint64, C.c_int, C.c_int, u64p, u64p, u64p]
    L.vx_shard_words.restype = None
    L.vx_shard_range.argtypes = [C.c_uint64, C.c_int, C.c_int, u64p, u64p]
    L.vx_shard_range.restype = None
    _lib = L
    return L


def _check(status):
    if status != VX_OK:
        raise VxError(status, lib().vx_last_error().decode("utf-8", "replace"))


def device_count():
    return lib().vx_device_count()


def set_device(d):
    _check(lib().vx_set_device(d))


def profile_enable(on=True):
    lib().vx_profile_enable(1 if on else 0)


def profile_select(kernel=None):
    """Time only this kernel (bare name); None = all kernels."""
    lib().vx_profile_select(kernel.encode() if kernel else None)


def profile_reset():
    lib().vx_profile_reset()


def profile_read():
    """{kernel base name: (total_ms, launches)} accumulated since the last reset (template arguments folded)."""
    out = {}
    slot = 0
    while True:
        name = C.create_string_buffer(128)
        ms, n = C.c_double(), C.c_uint64()
        if lib().vx_profile_read(slot, name, 128, C.byref(ms), C.byref(n)) != VX_OK:
            break
        key = name.value.decode().lstrip("(").split("<")[0].rstrip(")")
        a, b = out.get(key, (0.0, 0))
        out[key] = (a + ms.value, b + n.value)
        slot += 1
    return out


def morph_bit_radius():
    """vx_morph_bit_radius: the largest R = floor(sqrt(radius_sq)) the bit-level morphology kernel takes."""
    return int(lib().vx_morph_bit_radius())


def morph_radius_sq(radius=None, radius_sq=None):
    """radius (cells, may be fractional) -> radius_sq = floor(radius * radius) in float64; or radius_sq itself.  Exactly one of the two."""
    if (radius is None) == (radius_sq is None):
        raise ValueError("give exactly one of radius and radius_sq")
    if radius_sq is None:
        r = float(radius)
        if not (r >= 0.0) or r * r >= 4294967295.0:
            raise ValueError("radius out of range")
        return int(np.floor(r * r))
    r2 = int(radius_sq)
    if r2 < 0 or r2 > 0xFFFFFFFF:
        raise ValueError("radius_sq out of range")
    return r2


def device_allocations():
    """vx_device_allocations: device blocks requested from the library's pool so far (unchanged by a call that allocates nothing)."""
    return int(lib().vx_device_allocations())


def device_live_blocks():
    """vx_device_live_blocks: pool blocks held right now by handles and calls in progress, over all devices."""
    return int(lib().vx_device_live_blocks())


def pool_poison(pattern):
    """vx_pool_poison (a test aid): fill every block the pool hands out with the 32-bit `pattern` first; None switches the mode off."""
    if pattern is None:
        _check(lib().vx_pool_poison(0, 0))
    else:
        _check(lib().vx_pool_poison(1, int(pattern) & 0xFFFFFFFF))


def pool_poisoned_blocks():
    """vx_pool_poisoned_blocks: blocks the poison mode has filled since the library was loaded."""
    return int(lib().vx_pool_poisoned_blocks())


def shard_words(num_words, rank, world):
    b, e, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib().vx_shard_words(num_words, rank, world, C.byref(b), C.byref(e), C.byref(p))
    return b.value, e.value, p.value


def shard_range(count, rank, world):
    b, e = C.c_uint64(), C.c_uint64()
    lib().vx_shard_range(count, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


class _Handle:
    """What the handle classes share: `h`, the name of the C free function, an idempotent free() and a __del__ that swallows exceptions.
    owned = False (BorrowedGrid): free() only forgets the handle."""
    h = None
    owned = True
    _free = None

    def free(self):
        if self.h and self.owned:
            getattr(lib(), self._free)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Mesh(_Handle):
    """vx_mesh handle (what VoxelBuilder keeps after readObjFile)."""
    _free = "vx_mesh_free"

    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep

    @classmethod
    def load_obj(cls, path):
        h = C.c_void_p()
        _check(lib().vx_mesh_load_obj(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, verts, tris):
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        h = C.c_void_p()
        _check(lib().vx_mesh_from_arrays(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, verts_ptr, nverts, tris_ptr, ntris, keep=None):
        h = C.c_void_p()
        _check(lib().vx_mesh_from_device(verts_ptr, nverts, tris_ptr, ntris, C.byref(h)))
        return cls(h, keep)

    @property
    def num_vertices(self):
        return lib().vx_mesh_num_vertices(self.h)

    @property
    def num_triangles(self):
        return lib().vx_mesh_num_triangles(self.h)

    def host_arrays(self):
        nv, nt = self.num_vertices, self.num_triangles
        vp_, ip_ = lib().vx_mesh_host_vertices(self.h), lib().vx_mesh_host_indices(self.h)
        v = np.ctypeslib.as_array(C.cast(vp_, C.POINTER(C.c_float)), shape=(nv * 3,)).reshape(nv, 3).copy() if nv else np.zeros((0, 3), np.float32)
        t = np.ctypeslib.as_array(C.cast(ip_, C.POINTER(C.c_int32)), shape=(nt * 3,)).reshape(nt, 3).copy() if nt else np.zeros((0, 3), np.int32)
        return v, t

    def materials(self):
        """(records MATERIAL[n], per-triangle ids int32[T] or None): tinyobj's GetMaterials() / mesh.material_ids."""
        n = lib().vx_mesh_num_materials(self.h)
        recs = np.zeros(n, dtype=MATERIAL)
        if n:
            _check(lib().vx_mesh_materials(self.h, recs.ctypes.data, n))
        ip_ = lib().vx_mesh_host_material_ids(self.h)
        nt = self.num_triangles
        ids = np.ctypeslib.as_array(C.cast(ip_, C.POINTER(C.c_int32)), shape=(nt,)).copy() if (ip_ and nt) else None
        return recs, ids

    def bvh(self, max_leaf=0, stream=None):
        """vx_bvh_build: the triangle BVH of this mesh (max_leaf 0 = the library default)."""
        return Bvh(self, max_leaf, stream)

    def set_materials(self, records, tri_ids):
        r = np.ascontiguousarray(records, dtype=MATERIAL)
        ids = None if tri_ids is None else np.ascontiguousarray(tri_ids, dtype=np.int32)
        _check(lib().vx_mesh_set_materials(self.h, r.ctypes.data if r.size else None, r.size, ids.ctypes.data if ids is not None else None))

    def _host_f32(self, ptr, per_tri):
        nt = self.num_triangles
        if not ptr or not nt:
            return None
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(nt * per_tri,)).reshape(nt, 3, per_tri // 3).copy()

    def corner_normals(self):
        """float32[T, 3, 3] (corner k of triangle t: [t, k]) or None when the mesh has no corner normals"""
        return self._host_f32(lib().vx_mesh_host_corner_normals(self.h), 9)

    def corner_uvs(self):
        """float32[T, 3, 2] (uv = (u, 1 - v) of the OBJ) or None when the mesh has no corner uvs"""
        return self._host_f32(lib().vx_mesh_host_corner_uvs(self.h), 6)

    def set_attributes(self, normals=None, uvs=None):
        """vx_mesh_set_attributes: corner normals [T, 3, 3] and / or uvs [T, 3, 2]; None removes that attribute"""
        nt = self.num_triangles
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(nt * 9)
        u = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(nt * 6)
        _check(lib().vx_mesh_set_attributes(self.h, n.ctypes.data if n is not None else None, u.ctypes.data if u is not None else None))

    def texture_names(self):
        """the file of every texture slot (map_Kd, relative to the MTL's directory); "" for a slot set by set_texture"""
        return [lib().vx_mesh_texture_name(self.h, k).decode("utf-8", "replace") for k in range(lib().vx_mesh_num_textures(self.h))]

    def material_textures(self):
        """int32[num_materials]: the texture slot of every material (-1 none), or None without materials"""
        n = lib().vx_mesh_num_materials(self.h)
        p = lib().vx_mesh_host_material_textures(self.h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n,)).copy() if (p and n) else None

    def set_material_textures(self, slots):
        a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        _check(lib().vx_mesh_set_material_textures(self.h, a.ctypes.data if a.size else None, a.size))

    def texture(self, slot):
        """uint8[H, W, 4] (RGBA8, top row first) of a slot, or None when the slot has no image"""
        w, h = C.c_uint32(), C.c_uint32()
        p = lib().vx_mesh_host_texture(self.h, slot, C.byref(w), C.byref(h))
        if not p:
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(h.value * w.value * 4,)).reshape(h.value, w.value, 4).copy()

    def set_texture(self, slot, rgba):
        """vx_mesh_set_texture: rgba uint8[H, W, 4] (or [H, W, 3]: alpha 255), top row first"""
        a = np.asarray(rgba, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError("rgba must be [H, W, 4] or [H, W, 3]")
        if a.shape[2] == 3:
            a = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], 2)
        a = np.ascontiguousarray(a)
        _check(lib().vx_mesh_set_texture(self.h, int(slot), a.shape[1], a.shape[0], a.ctypes.data))

    def load_textures(self):
        """vx_mesh_load_textures: decode every slot's file (PPM P6 / TGA; 1x1 magenta where that fails)"""
        _check(lib().vx_mesh_load_textures(self.h))


class Grid(_Handle):
    """vx_grid handle (a VoxelGridBool / VoxelGridAABBstruct / VoxelGridVec)."""
    _free = "vx_grid_free"

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def voxelize(cls, mesh, voxel_size, kind=GRID_BOOL, sat_variant=0, words=None, tris=None, stream=None, materials=False, shard=None, solid=False):
        o = VoxelizeOpts()
        o.sat_variant = sat_variant
        o.flags = (VOXELIZE_MATERIALS if materials else 0) | (VOXELIZE_SOLID if solid else 0)
        if shard is not None:
            o.shard_rank, o.shard_world = shard
        if words is not None:
            o.word_begin, o.word_end = words
        if tris is not None:
            o.tri_begin, o.tri_end = tris
        o.stream = stream
        h = C.c_void_p()
        _check(lib().vx_voxelize(mesh.h, np.float32(voxel_size), kind, C.byref(o), C.byref(h)))
        g = cls(h)
        g._stream = stream
        return g

    @classmethod
    def voxelize_multi(cls, mesh, voxel_size, devices, kind=GRID_BOOL, sat_variant=0, all_gather=False):
        """vx_voxelize_multi: word shards on the given devices + peer copies -> [grid on devices[0]] or one grid per device."""
        dv = (C.c_int * len(devices))(*devices)
        n = len(devices) if all_gather else 1
        hs = (C.c_void_p * n)()
        _check(lib().vx_voxelize_multi(mesh.h, np.float32(voxel_size), kind, sat_variant, dv, len(devices), 1 if all_gather else 0, hs))
        return [cls(C.c_void_p(hs[i])) for i in range(n)]

    def revoxelize(self, mesh, voxel_size, sat_variant=0, words=None, tris=None, stream=None, materials=False, shard=None, list_async=False,
                   solid=False):
        o = VoxelizeOpts()
        o.sat_variant = sat_variant
        o.flags = (VOXELIZE_MATERIALS if materials else 0) | (VOXELIZE_LIST_ASYNC if list_async else 0) | (VOXELIZE_SOLID if solid else 0)
        if shard is not None:
            o.shard_rank, o.shard_world = shard
        if words is not None:
            o.word_begin, o.word_end = words
        if tris is not None:
            o.tri_begin, o.tri_end = tris
        o.stream = stream
        self._stream = stream
        _check(lib().vx_voxelize_into(mesh.h, np.float32(voxel_size), C.byref(o), self.h))

    @classmethod
    def create(cls, kind, x, y, z, voxel_size, origin=(0.0, 0.0, 0.0), stream=None):
        org = (C.c_float * 3)(*origin)
        h = C.c_void_p()
        _check(lib().vx_grid_create(kind, x, y, z, np.float32(voxel_size), org, stream, C.byref(h)))
        g = cls(h)
        g._stream = stream
        return g

    def describe(self):
        d = GridDesc()
        _check(lib().vx_grid_describe(self.h, C.byref(d)))
        return dict(dim=tuple(int(x) for x in d.dim), voxel_size=float(d.voxel_size), origin=np.array(d.origin, np.float32),
                    bbox_min=np.array(d.bbox_min, np.float32), bbox_max=np.array(d.bbox_max, np.float32),
                    bbox_center=np.array(d.bbox_center, np.float32), num_words=int(d.num_words), set_calls=int(d.set_calls),
                    occupied=int(d.occupied), triangles=int(d.triangles), kind=int(d.kind), device=int(d.device))

    def set_voxel(self, x, y, z):
        _check(lib().vx_grid_set_voxel(self.h, x, y, z))

    def test_voxel(self, x, y, z):
        r = C.c_int()
        _check(lib().vx_grid_test_voxel(self.h, x, y, z, C.byref(r)))
        return bool(r.value)

    def coords(self, x, y, z):
        o = (C.c_float * 3)()
        _check(lib().vx_grid_coords(self.h, x, y, z, o))
        return np.array(o, dtype=np.float32)

    def memory_bytes(self):
        return int(lib().vx_grid_bytes(self.h))

    def bitmask(self):
        n = self.describe()["num_words"]
        w = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().vx_grid_bitmask(self.h, w.ctypes.data, n))
        return w[:n]

    def bitmask_device_ptr(self, mutable=False):
        return lib().vx_grid_bitmask_device_mut(self.h) if mutable else lib().vx_grid_bitmask_device(self.h)

    def refresh(self):
        _check(lib().vx_grid_refresh(self.h))

    def fill_interior(self):
        """vx_grid_fill_interior: setVoxel on every enclosed empty cell (6-connected exterior), ascending; returns the count."""
        _check(lib().vx_grid_fill_interior(self.h))
        return self.interior()

    def interior(self):
        """|H| of the last solid build or fill_interior on this handle (0 otherwise)."""
        n = C.c_uint64()
        _check(lib().vx_grid_interior(self.h, C.byref(n)))
        return int(n.value)

    def fill_rounds(self):
        """Flood-fill rounds of the last solid build or fill_interior, the final quiet round included."""
        return int(lib().vx_grid_fill_rounds(self.h))

    def _cells(self):
        x, y, z = self.describe()["dim"]
        return (z, y, x), x * y * z

    def distance_sq(self, inside=False):
        """vx_grid_distance_sq: the exact squared distance (cell units) of every cell to the nearest occupied cell (inside=True: to the
        nearest empty cell) -> numpy uint32 [Z, Y, X]; 0xFFFFFFFF where no such cell exists."""
        shape, n = self._cells()
        out = np.zeros(shape, dtype=np.uint32)
        _check(lib().vx_grid_distance_sq(self.h, DISTANCE_INSIDE if inside else 0, out.ctypes.data, n))
        return out

    def sdf(self):
        """vx_grid_sdf: the signed distance field -> numpy float32 [Z, Y, X]; vs * sqrt(D_out) off the mask, -vs * sqrt(D_in) on it."""
        shape, n = self._cells()
        out = np.zeros(shape, dtype=np.float32)
        _check(lib().vx_grid_sdf(self.h, out.ctypes.data, n))
        return out

    def _device_out(self, out, dtypes, name):
        import torch
        shape, n = self._cells()
        if out is None:
            out = torch.empty(shape, dtype=dtypes[0], device="cuda")
        if out.dtype not in dtypes or out.numel() != n or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous device %s tensor of X*Y*Z elements" % name)
        return out, n

    def _record(self, out):
        """the caching allocator must not hand `out` out again before the grid's stream has written it"""
        import torch
        st = getattr(self, "_stream", None)
        if hasattr(st, "cuda_stream"):
            out.record_stream(st)
        elif st:
            out.record_stream(torch.cuda.ExternalStream(st))
        else:
            out.record_stream(torch.cuda.default_stream(out.device))

    def distance_sq_device(self, out=None, inside=False):
        """vx_grid_distance_sq_device, asynchronous on the grid's stream -> `out`, a device torch.uint32 tensor [Z, Y, X] (an int32
        tensor receives the same bits)."""
        import torch
        out, n = self._device_out(out, (torch.uint32, torch.int32), "uint32 / int32")
        _check(lib().vx_grid_distance_sq_device(self.h, DISTANCE_INSIDE if inside else 0, out.data_ptr(), n))
        self._record(out)
        return out

    def sdf_device(self, out=None):
        """vx_grid_sdf_device, asynchronous on the grid's stream -> `out`, a device torch.float32 tensor [Z, Y, X]."""
        import torch
        out, n = self._device_out(out, (torch.float32,), "float32")
        _check(lib().vx_grid_sdf_device(self.h, out.data_ptr(), n))
        self._record(out)
        return out

    def field(self, stream=None):
        """vx_field_create: a snapshot of the signed field that stays on the device, for queries at the caller's own points -> Field.
        `stream`: the stream of the field's queries.  The field does not depend on the grid afterwards."""
        h = C.c_void_p()
        _check(lib().vx_field_create(self.h, _stream_handle(stream), C.byref(h)))
        return Field(h)

    def nearest(self, inside=False):
        """vx_grid_nearest: the cell index x + X*(y + Y*z) of every cell's nearest occupied cell (inside=True: nearest empty cell), the
        smallest index among equally near ones -> numpy uint32 [Z, Y, X]; 0xFFFFFFFF where no such cell exists."""
        shape, n = self._cells()
        out = np.zeros(shape, dtype=np.uint32)
        _check(lib().vx_grid_nearest(self.h, DISTANCE_INSIDE if inside else 0, out.ctypes.data, n))
        return out

    def nearest_device(self, out=None, inside=False):
        """vx_grid_nearest_device, asynchronous on the grid's stream -> `out`, a device torch.uint32 tensor [Z, Y, X] (an int32 tensor
        receives the same bits)."""
        import torch
        out, n = self._device_out(out, (torch.uint32, torch.int32), "uint32 / int32")
        _check(lib().vx_grid_nearest_device(self.h, DISTANCE_INSIDE if inside else 0, out.data_ptr(), n))
        self._record(out)
        return out

    def nearest_gather(self, values, fill=0, inside=False):
        """vx_grid_nearest_gather: values[nearest()] per cell, `fill` where there is no nearest cell -> numpy uint32 [Z, Y, X].  `values`:
        one uint32 per cell, [Z, Y, X] or flat."""
        shape, n = self._cells()
        values = np.ascontiguousarray(values, dtype=np.uint32)
        if values.size != n:
            raise ValueError("values must hold X*Y*Z elements")
        out = np.zeros(shape, dtype=np.uint32)
        _check(lib().vx_grid_nearest_gather(self.h, DISTANCE_INSIDE if inside else 0, values.ctypes.data, n, int(fill) & 0xFFFFFFFF,
                                            out.ctypes.data, n))
        return out

    def nearest_gather_device(self, values, out=None, fill=0, inside=False):
        """vx_grid_nearest_gather_device, asynchronous on the grid's stream: `values`, a contiguous device uint32 / int32 tensor of X*Y*Z
        elements written on (or ordered before) that stream -> `out`, a different tensor of the same kind."""
        import torch
        out, n = self._device_out(out, (torch.uint32, torch.int32), "uint32 / int32")
        if values.dtype not in (torch.uint32, torch.int32) or values.numel() != n or not values.is_contiguous() or not values.is_cuda:
            raise ValueError("values must be a contiguous device uint32 / int32 tensor of X*Y*Z elements")
        _check(lib().vx_grid_nearest_gather_device(self.h, DISTANCE_INSIDE if inside else 0, values.data_ptr(), n, int(fill) & 0xFFFFFFFF,
                                                   out.data_ptr(), n))
        self._record(values)
        self._record(out)
        return out

    def nearest_labels(self, connectivity=CONNECT_6):
        """The Voronoi partition of the grid by part: every cell gets the component label (components(connectivity)) of its nearest
        occupied cell -> (numpy uint32 [Z, Y, X], K); all 0 when nothing is occupied.  components_device, then nearest_gather_device, on
        the grid's stream, with one host wait."""
        import torch
        shape, n = self._cells()
        if not n:
            return np.zeros(shape, dtype=np.uint32), 0
        lab, k = self.components_device(connectivity=connectivity)
        out = self.nearest_gather_device(lab, fill=0)
        st = getattr(self, "_stream", None)
        with torch.cuda.stream(st if hasattr(st, "cuda_stream") else torch.cuda.ExternalStream(st) if st else torch.cuda.default_stream()):
            host = torch.cat([out.view(torch.int32).reshape(-1), k.reshape(-1)]).cpu().numpy()  # (on the grid's stream: the one host wait)
        return host[:-1].view(np.uint32).reshape(tuple(out.shape)).copy(), int(host[-1])

    def _morph_grid(self, op, radius, radius_sq):
        h = C.c_void_p()
        r2 = morph_radius_sq(radius, radius_sq)
        if op is None:
            _check(lib().vx_grid_seal(self.h, r2, C.byref(h)))
        else:
            _check(lib().vx_grid_morph(self.h, op, r2, C.byref(h)))
        g = Grid(h)
        g._stream = getattr(self, "_stream", None)
        return g

    def dilate(self, radius=None, radius_sq=None):
        """vx_grid_morph(VX_MORPH_DILATE): a new Grid, this one grown by the Euclidean ball of `radius` cells (fractional radii allowed:
        radius_sq = floor(radius^2); radius=1.5 is the 18-neighbourhood).  Exactly one of radius / radius_sq."""
        return self._morph_grid(MORPH_DILATE, radius, radius_sq)

    def erode(self, radius=None, radius_sq=None):
        """vx_grid_morph(VX_MORPH_ERODE): a new Grid of the cells whose whole ball lies in this one (cells outside the grid are empty)."""
        return self._morph_grid(MORPH_ERODE, radius, radius_sq)

    def open(self, radius=None, radius_sq=None):
        """vx_grid_morph(VX_MORPH_OPEN): erosion, then dilation -- drops specks; a subset of this grid."""
        return self._morph_grid(MORPH_OPEN, radius, radius_sq)

    def close(self, radius=None, radius_sq=None):
        """vx_grid_morph(VX_MORPH_CLOSE): dilation on the unbounded lattice, then erosion -- fills gaps narrower than the ball; a superset."""
        return self._morph_grid(MORPH_CLOSE, radius, radius_sq)

    def seal(self, radius=None, radius_sq=None):
        """vx_grid_seal: this grid plus the interior that appears once holes up to the ball's size are closed (dilate, fill, erode); the
        result's interior() is the number of cells added."""
        return self._morph_grid(None, radius, radius_sq)

    def morph_mask(self, op, radius_sq):
        """vx_grid_morph_mask: the result of MORPH_* `op` as numpy uint32 words in this grid's own layout."""
        n = self.describe()["num_words"]
        w = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().vx_grid_morph_mask(self.h, op, radius_sq, w.ctypes.data, n))
        return w[:n]

    def morph_mask_device(self, op, radius_sq, out=None):
        """vx_grid_morph_device, asynchronous on the grid's stream -> `out`, a device torch.uint32 (or int32) tensor of num_words words."""
        import torch
        n = self.describe()["num_words"]
        if out is None:
            out = torch.empty(n, dtype=torch.uint32, device="cuda")
        if out.dtype not in (torch.uint32, torch.int32) or out.numel() < n or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous device uint32 / int32 tensor of at least num_words elements")
        _check(lib().vx_grid_morph_device(self.h, op, radius_sq, out.data_ptr(), out.numel()))
        self._record(out)
        return out

    def surface_counts(self, materials=False):
        """(V, T) of the boundary mesh (vx_grid_surface size query; materials=True also checks that the grid has per-cell ids)."""
        nv, nt = C.c_uint64(), C.c_uint64()
        probe = np.zeros(1, np.int32)
        _check(lib().vx_grid_surface(self.h, None, 0, None, 0, probe.ctypes.data if materials else None, C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def _surface_arrays(self, counts, device, materials, normals, sp=None):
        """(verts, tris[, mats][, normals]) for counts = (V, T): numpy arrays from the host entry point, or device torch tensors from the
        _device one, recorded on the grid's stream.  sp: the vx_smooth of the surface nets; None: the faces' mesh."""
        nv, nt = counts
        if device:
            import torch

            def new(shape, dtype):
                return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")
        else:
            def new(shape, dtype):
                return np.zeros(shape, getattr(np, dtype))
        v, t = new((nv, 3), "float32"), new((nt, 3), "int32")
        out = (v, t) + ((new(nt, "int32"),) if materials else ()) + ((new((nv, 3), "float32"),) if normals else ())
        if nv or nt:
            ptr = [x.data_ptr() if device else x.ctypes.data for x in out]
            args = [ptr[0], nv, ptr[1], nt, ptr[2] if materials else None]
            if sp is not None:
                args = [C.byref(sp)] + args + [ptr[-1] if normals else None]
            a, b = C.c_uint64(), C.c_uint64()
            entry = "vx_grid_surface" + ("_smooth" if sp is not None else "") + ("_device" if device else "")
            _check(getattr(lib(), entry)(self.h, *args, C.byref(a), C.byref(b)))
            if device:
                for x in out:
                    self._record(x)
        return out

    def surface(self, materials=False):
        """vx_grid_surface: the boundary mesh of the occupancy -> (verts (V, 3) float32, tris (T, 3) int32[, mats (T,) int32])."""
        return self._surface_arrays(self.surface_counts(materials), False, materials, False)

    def surface_device(self, materials=False):
        """vx_grid_surface_device: the same arrays as device torch tensors, written asynchronously on the grid's stream (the host waits
        for the two counts only)."""
        return self._surface_arrays(self.surface_counts(materials), True, materials, False)

    def surface_mesh(self, materials=False):
        """vx_grid_surface_mesh: the boundary mesh as a Mesh (with materials: the grid's records and one id per triangle)."""
        h = C.c_void_p()
        _check(lib().vx_grid_surface_mesh(self.h, 1 if materials else 0, C.byref(h)))
        return Mesh(h)

    def _smooth_counts(self, iterations, lam, mu, materials):
        """(vx_smooth, V, T): vx_grid_surface_smooth's size query, which also checks the parameters and, with materials, the ids"""
        sp = Smooth(iterations, lam, mu)
        nv, nt = C.c_uint64(), C.c_uint64()
        probe = np.zeros(1, np.int32)
        _check(lib().vx_grid_surface_smooth(self.h, C.byref(sp), None, 0, None, 0, probe.ctypes.data if materials else None, None, C.byref(nv),
                                            C.byref(nt)))
        return sp, nv.value, nt.value

    def surface_smooth(self, iterations=8, lam=0.5, mu=-0.53, materials=False, normals=False):
        """vx_grid_surface_smooth: the surface-nets mesh -> (verts (V, 3) float32, tris (T, 3) int32[, mats (T,) int32][, normals (V, 3)
        float32]): vx_grid_surface's vertices and triangles, the positions relaxed by `iterations` x (a step with lam, a step with mu)."""
        sp, nv, nt = self._smooth_counts(iterations, lam, mu, materials)
        return self._surface_arrays((nv, nt), False, materials, normals, sp)

    def surface_smooth_device(self, iterations=8, lam=0.5, mu=-0.53, materials=False, normals=False):
        """vx_grid_surface_smooth_device: the same arrays as device torch tensors, written asynchronously on the grid's stream (the host
        waits for the two counts only)."""
        sp, nv, nt = self._smooth_counts(iterations, lam, mu, materials)
        return self._surface_arrays((nv, nt), True, materials, normals, sp)

    def surface_smooth_mesh(self, iterations=8, lam=0.5, mu=-0.53, materials=False, normals=False):
        """vx_grid_surface_smooth_mesh: the surface-nets mesh as a Mesh (with normals: corner normals from the vertex normals, so an
        attributes renderer shades it smoothly)."""
        sp = Smooth(iterations, lam, mu)
        h = C.c_void_p()
        _check(lib().vx_grid_surface_smooth_mesh(self.h, C.byref(sp), 1 if materials else 0, 1 if normals else 0, C.byref(h)))
        return Mesh(h)

    def components(self, connectivity=CONNECT_6):
        """vx_grid_components: connected-component labels of the occupied cells (connectivity 6 or 26) -> (numpy uint32 [Z, Y, X], K);
        0 for empty cells, 1..K in ascending order of each component's smallest cell index."""
        shape, n = self._cells()
        out = np.zeros(shape, dtype=np.uint32)
        k = C.c_uint64()
        _check(lib().vx_grid_components(self.h, connectivity, out.ctypes.data if n else None, n, C.byref(k)))
        return out, k.value

    def components_device(self, out=None, connectivity=CONNECT_6):
        """vx_grid_components_device, asynchronous on the grid's stream -> (`out`, a device torch.uint32 tensor [Z, Y, X] of labels (an int32
        tensor receives the same bits), K as a one-element device int32 tensor)."""
        import torch
        out, n = self._device_out(out, (torch.uint32, torch.int32), "uint32 / int32")
        if not n:
            return out, torch.zeros(1, dtype=torch.int32, device=out.device)
        k = torch.empty(1, dtype=torch.int32, device=out.device)
        _check(lib().vx_grid_components_device(self.h, connectivity, out.data_ptr(), n, k.data_ptr()))
        self._record(out)
        self._record(k)
        return out, k

    def component_stats(self, connectivity=CONNECT_6):
        """vx_grid_component_stats -> numpy COMPONENT[K]: record k - 1 describes label k (cells, inclusive min / max cell in x, y, z)."""
        k = C.c_uint64()
        _check(lib().vx_grid_component_stats(self.h, connectivity, None, 0, C.byref(k)))
        out = np.zeros(k.value, dtype=COMPONENT)
        if k.value:
            _check(lib().vx_grid_component_stats(self.h, connectivity, out.ctypes.data, k.value, C.byref(k)))
        return out

    def aabbs(self):
        n = C.c_uint64()
        _check(lib().vx_grid_aabbs(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=AABB)
        if n.value:
            _check(lib().vx_grid_aabbs(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def material_first_use(self):
        """Sharded VX_VOXELIZE_MATERIALS build: per material value the first triangle of this shard that uses it (-1: none)."""
        n = C.c_uint64()
        _check(lib().vx_grid_material_first_use(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        _check(lib().vx_grid_material_first_use(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), n.value, None))
        return out[:n.value]

    def finish_materials(self, first_use_min):
        fu = np.ascontiguousarray(first_use_min, dtype=np.int64)
        _check(lib().vx_grid_finish_materials(self.h, fu.ctypes.data_as(C.POINTER(C.c_int64)), fu.size))

    def materials(self):
        """(getMatrials() as MATERIAL records, getMatIdx() as int16[]) -- empty unless built with materials=True."""
        n = C.c_uint64()
        _check(lib().vx_grid_materials(self.h, None, 0, C.byref(n)))
        recs = np.zeros(n.value, dtype=MATERIAL)
        if n.value:
            _check(lib().vx_grid_materials(self.h, recs.ctypes.data, n.value, C.byref(n)))
        _check(lib().vx_grid_material_ids(self.h, None, 0, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.int16)
        if n.value:
            _check(lib().vx_grid_material_ids(self.h, ids.ctypes.data, n.value, C.byref(n)))
        return recs, ids

    def bind_aabbs_device(self, dev_ptr, capacity):
        """VX_GRID_VEC: later revoxelize() calls build the list straight in this device buffer (None / 0 removes the binding)."""
        _check(lib().vx_grid_bind_aabbs_device(self.h, dev_ptr, capacity))

    def list_wait(self):
        """VX_VOXELIZE_LIST_ASYNC builds: work queued on the grid's stream after this call sees the complete list."""
        _check(lib().vx_grid_list_wait(self.h))

    def aabbs_device_async(self, dev_ptr, capacity):
        """vx_grid_aabbs_device_async: the count now, the records beside the next ray batch (or after list_wait())."""
        n = C.c_uint64()
        _check(lib().vx_grid_aabbs_device_async(self.h, dev_ptr, capacity, C.byref(n)))
        return n.value

    def aabbs_device(self, dev_ptr, capacity):
        n = C.c_uint64()
        _check(lib().vx_grid_aabbs_device(self.h, dev_ptr, capacity, C.byref(n)))
        return n.value

    def trace(self, rays, tmin=0.001, tmax=10000.0, want_prim=True):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        t = np.zeros(r.shape[0], dtype=np.float32)
        p = np.zeros(r.shape[0], dtype=np.uint32) if want_prim else None
        nh = C.c_uint64()
        _check(lib().vx_trace(self.h, r.ctypes.data, r.shape[0], np.float32(tmin), np.float32(tmax), t.ctypes.data,
                              p.ctypes.data if want_prim else None, C.byref(nh)))
        return (t, p, nh.value) if want_prim else (t, nh.value)

    def trace_ex(self, rays=None, camera=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, any_hit=False, want=("t", "prim")):
        """Host-buffer extended query -> dict of the requested outputs (t, prim, normal, shadowed)."""
        return _trace_ex(lib().vx_trace_ex, self.h, TraceArgs(), rays, camera, tmin, tmax, tmax_per_ray, any_hit, want)

    def trace_device(self, rays_ptr, nrays, t_ptr, prim_ptr=None, hits_ptr=None, nhits_ptr=None, tmin=0.001, tmax=10000.0):
        _check(lib().vx_trace_device(self.h, rays_ptr, nrays, np.float32(tmin), np.float32(tmax), t_ptr, prim_ptr, hits_ptr, nhits_ptr))

    def trace_multi(self, rays=None, camera=None, max_hits=8, tmin=0.001, tmax=10000.0, tmax_per_ray=None, after=None, want=("t", "prim", "count")):
        """vx_trace_multi on host arrays: per ray the first max_hits accepted hits in (t, prim) order and the number of all of them -> dict
        of the requested outputs: t (n, K) float32 and prim (n, K) uint32, padded with -1 / 0xFFFFFFFF, count (n,) uint32.  after =
        (after_t, after_prim): per-ray cursor, only hits strictly behind it are listed and counted."""
        return _trace_multi(lib().vx_trace_multi, self.h, MultiHitArgs(), 2, rays, camera, max_hits, tmin, tmax, tmax_per_ray, after, want)

    def trace_multi_device(self, rays_ptr, nrays, max_hits, t_ptr=None, prim_ptr=None, count_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None,
                           after_t_ptr=None, after_prim_ptr=None, camera=None):
        """vx_trace_multi_device on raw device pointers, asynchronous on the grid's stream; t / prim hold max_hits entries per ray.
        camera = (view_inv, proj_inv, width, height) in place of rays_ptr / nrays."""
        _trace_multi_device(lib().vx_trace_multi_device, self.h, MultiHitArgs(), rays_ptr, nrays, camera, max_hits, tmin, tmax, t=t_ptr, prim=prim_ptr,
                            count=count_ptr, tmax_per_ray=tmax_per_ray_ptr, after_t=after_t_ptr, after_prim=after_prim_ptr)

    def trace_primary_device(self, view_inv, proj_inv, width, height, t_ptr, prim_ptr=None, tmin=0.001, tmax=10000.0):
        a = TraceArgs()
        _ray_batch(a, None, (view_inv, proj_inv, width, height), tmin, tmax, None, [])
        _check(lib().vx_trace_primary_device(self.h, a.view_inverse, a.proj_inverse, a.width, a.height, a.tmin, a.tmax, t_ptr, prim_ptr))


FIELD_FINITE, FIELD_EMPTY, FIELD_FULL = 0, 1, 2
FIELD_MISS, FIELD_HIT, FIELD_STEP_LIMIT = 0, 1, 2
# the outputs of the field queries, as _FIRST_HIT
_FIELD_SAMPLE = {"value": ((), np.float32), "gradient": ((3,), np.float32), "occupied": ((), np.uint8)}
_FIELD_TRACE = {"t": ((), np.float32), "clearance": ((), np.float32), "steps": ((), np.uint32), "status": ((), np.uint8)}
_FIELD_POSES = {"clearance": ((), np.float32), "point": ((), np.uint32), "count": ((), np.uint32), "position": ((3,), np.float32),
                "gradient": ((3,), np.float32)}
POSE_CHUNK, POSE_TILE = 256, 32   # VX_FIELD_POSE_CHUNK / _TILE: how the pose kernel cuts a body of more than 64 points (no result shows it)
POSE_NO_POINT = 0xFFFFFFFF


class Field(_Handle):
    """vx_field handle: a device-resident snapshot of a grid's signed distance field, sampled trilinearly at arbitrary points and sphere
    traced along rays (include/voxhip.h, "distance-field queries")."""
    _free = "vx_field_free"

    def __init__(self, handle):
        self.h = handle

    def update(self, grid):
        """vx_field_update: re-snapshots a grid of the same dimensions into the same buffer."""
        _check(lib().vx_field_update(self.h, grid.h))

    def describe(self):
        d = FieldDesc()
        _check(lib().vx_field_describe(self.h, C.byref(d)))
        return dict(dim=tuple(int(x) for x in d.dim), voxel_size=float(d.voxel_size), origin=np.array(d.origin, np.float32), state=int(d.state),
                    bytes=int(d.bytes))

    def values_device_ptr(self):
        """the snapshot on the device: X*Y*Z float32 at x + X*(y + Y*z), exactly sdf()'s values"""
        return lib().vx_field_values_device(self.h)

    def sample(self, points, want=("value", "gradient", "occupied")):
        """vx_field_sample on host points (n, 3) -> dict of the requested outputs: value (n,) float32, gradient (n, 3) float32, occupied
        (n,) uint8."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        a = FieldSampleArgs()
        a.points, a.num_points = p.ctypes.data, p.shape[0]
        out = _outputs(a, want, p.shape[0], _FIELD_SAMPLE)
        _check(lib().vx_field_sample(self.h, C.byref(a)))
        return out

    def sample_device(self, points_ptr, n, value_ptr=None, gradient_ptr=None, occupied_ptr=None):
        """vx_field_sample_device on raw device pointers, asynchronous on the field's stream."""
        a = FieldSampleArgs()
        a.points, a.num_points = points_ptr, n
        _set_pointers(a, dict(value=value_ptr, gradient=gradient_ptr, occupied=occupied_ptr))
        _check(lib().vx_field_sample_device(self.h, C.byref(a)))

    @staticmethod
    def _trace_args(rays_ptr, n, radius, tmin, tmax, step_scale, hit_eps, max_steps):
        a = FieldTraceArgs()
        a.rays, a.num_rays = rays_ptr, n
        a.tmin, a.tmax, a.radius = np.float32(tmin), np.float32(tmax), np.float32(radius)
        a.step_scale, a.hit_eps, a.max_steps = np.float32(step_scale), np.float32(hit_eps), int(max_steps)
        return a

    def sphere_trace(self, rays, radius=0.0, radius_per_ray=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, step_scale=0.25, hit_eps=1.0 / 64,
                     max_steps=256, want=("t", "clearance", "steps", "status")):
        """vx_field_sphere_trace on host rays (n, 6): a sphere of `radius` (world units) moved along each ray until the field at its centre
        is within hit_eps cells of the radius -> dict of the requested outputs: t (n,) float32 (-1: no hit), clearance (n,) float32 (the
        smallest field value met), steps (n,) uint32, status (n,) uint8 (FIELD_MISS / FIELD_HIT / FIELD_STEP_LIMIT)."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        a = self._trace_args(r.ctypes.data, r.shape[0], radius, tmin, tmax, step_scale, hit_eps, max_steps)
        keep = [np.ascontiguousarray(x, dtype=np.float32) if x is not None else None for x in (tmax_per_ray, radius_per_ray)]
        for name, x in zip(("tmax_per_ray", "radius_per_ray"), keep):
            if x is not None:
                if x.shape != (r.shape[0],):
                    raise ValueError("%s has one entry per ray" % name)
                setattr(a, name, x.ctypes.data)
        out = _outputs(a, want, r.shape[0], _FIELD_TRACE)
        _check(lib().vx_field_sphere_trace(self.h, C.byref(a)))
        return out

    def sphere_trace_device(self, rays_ptr, nrays, radius=0.0, radius_per_ray_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None, step_scale=0.25,
                            hit_eps=1.0 / 64, max_steps=256, t_ptr=None, clearance_ptr=None, steps_ptr=None, status_ptr=None):
        """vx_field_sphere_trace_device on raw device pointers, asynchronous on the field's stream."""
        a = self._trace_args(rays_ptr, nrays, radius, tmin, tmax, step_scale, hit_eps, max_steps)
        _set_pointers(a, dict(radius_per_ray=radius_per_ray_ptr, tmax_per_ray=tmax_per_ray_ptr, t=t_ptr, clearance=clearance_ptr, steps=steps_ptr,
                              status=status_ptr))
        _check(lib().vx_field_sphere_trace_device(self.h, C.byref(a)))

    def poses(self, points, transforms, radii=None, margin=0.0, want=("clearance", "point", "count")):
        """vx_field_poses: a body of host points (P, 3) with optional radii (P,) under host transforms (N, 3, 4) (body to world, row-major)
        -> dict of the requested outputs, one entry per pose: clearance (N,) float32 (the smallest value - radius over the body; +inf: no
        point took part), point (N,) uint32 (which point; POSE_NO_POINT), count (N,) uint32 (points within `margin`), position (N, 3)
        and gradient (N, 3) float32 (the contact point and the normal out of the solid)."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        a = FieldPoseArgs()
        a.points, a.num_points = p.ctypes.data if p.shape[0] else None, p.shape[0]
        a.transforms, a.num_poses = m.ctypes.data if m.shape[0] else None, m.shape[0]
        a.margin = np.float32(margin)
        r = None
        if radii is not None:
            r = np.ascontiguousarray(radii, dtype=np.float32)
            if r.shape != (p.shape[0],):
                raise ValueError("radii has one entry per point")
            a.radii = r.ctypes.data if p.shape[0] else None
        out = _outputs(a, want, m.shape[0], _FIELD_POSES)
        _check(lib().vx_field_poses(self.h, C.byref(a)))
        return out

    def poses_device(self, points_ptr, num_points, transforms_ptr, num_poses, radii_ptr=None, margin=0.0, **output_ptrs):
        """vx_field_poses_device on raw device pointers, asynchronous on the field's stream; output_ptrs: clearance, point, count,
        position, gradient -> device pointer."""
        unknown = set(output_ptrs) - set(_FIELD_POSES)
        if unknown:
            raise ValueError("no such pose output: %s" % ", ".join(sorted(unknown)))
        a = FieldPoseArgs()
        a.points, a.num_points, a.transforms, a.num_poses = points_ptr, num_points, transforms_ptr, num_poses
        a.margin = np.float32(margin)
        _set_pointers(a, dict(radii=radii_ptr, **output_ptrs))
        _check(lib().vx_field_poses_device(self.h, C.byref(a)))


def sort_u64(keys, bits):
    """vx_sort_u64: the octree's device radix sort on a host array (returns a sorted copy)."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    _check(lib().vx_sort_u64(k.ctypes.data, k.size, int(bits)))
    return k


SCAN_MODES = {"values": 0, "popcount": 1, "bytes": 2}
SCAN_PATHS = {"gen": 0, "ticket": 1, "three": 2, "auto": 3}
SCAN_CANARY, SCAN_CANARY_VALUE = 16, 0xA5A5A5A5


def scan_u32(inputs, mode="values", paths="gen", in_offset=0, out_offset=0, sel_cap=0, group16_cap=0, total_tag=0, gen_start=0):
    """vx_scan_u32: the device prefix scan on host arrays, one scan per entry of `inputs`, all on one scratch block (voxhip.h).
    paths: one name of SCAN_PATHS or one per scan.  Returns one dict per scan: out (n + 1 uint32), canary (the SCAN_CANARY words
    behind out[n]), total (the 64-bit word as written), taken (the path's name), clean, and sel / group16 (sel_cap / group16_cap words
    each, when asked for)."""
    dt = np.uint8 if mode == "bytes" else np.uint32
    arrs = [np.ascontiguousarray(x, dtype=dt) for x in inputs]
    k = len(arrs)
    paths = [paths] * k if isinstance(paths, str) else list(paths)
    sizes = np.array([a.size for a in arrs], dtype=np.uint64)
    pth = np.array([SCAN_PATHS[p] for p in paths], dtype=np.uint32)
    inp = np.concatenate(arrs) if k else np.zeros(0, dt)
    if inp.size == 0:
        inp = np.zeros(1, dt)
    out = np.zeros(int(sizes.sum()) + k * (1 + SCAN_CANARY), dtype=np.uint32)
    totals = np.zeros(k, np.uint64)
    taken = np.zeros(k, np.uint32)
    clean = np.zeros(k, np.uint32)
    sel = np.zeros(max(k * sel_cap, 1), np.uint32)
    g16 = np.zeros(max(k * group16_cap, 1), np.uint32)
    a = ScanArgs(mode=SCAN_MODES[mode], nscans=k, sizes=sizes.ctypes.data, paths=pth.ctypes.data, inp=inp.ctypes.data, out=out.ctypes.data,
                 totals=totals.ctypes.data, taken=taken.ctypes.data, clean=clean.ctypes.data, sel=sel.ctypes.data if sel_cap else None,
                 group16=g16.ctypes.data if group16_cap else None, sel_cap=sel_cap, group16_cap=group16_cap, in_offset=in_offset,
                 out_offset=out_offset, total_tag=total_tag, gen_start=gen_start)
    _check(lib().vx_scan_u32(C.byref(a)))
    names = {v: n for n, v in SCAN_PATHS.items()}
    res, o = [], 0
    for i, x in enumerate(arrs):
        n = x.size
        r = dict(out=out[o:o + n + 1], canary=out[o + n + 1:o + n + 1 + SCAN_CANARY], total=int(totals[i]), taken=names[int(taken[i])],
                 clean=bool(clean[i]))
        if sel_cap:
            r["sel"] = sel[i * sel_cap:(i + 1) * sel_cap]
        if group16_cap:
            r["group16"] = g16[i * group16_cap:(i + 1) * group16_cap]
        res.append(r)
        o += n + 1 + SCAN_CANARY
    return res


class BorrowedGrid(Grid):
    """A grid owned by a vx_multi context (valid until its next voxelize / free)."""
    owned = False


class Multi(_Handle):
    """vx_multi handle: a mesh resident on several devices (logical ranks allowed), one grid and one worker thread per rank;
    voxelize() rebuilds the grid in steady state (word shards by rank + peer copies)."""
    _free = "vx_multi_free"

    def __init__(self, mesh, devices, kind=GRID_BOOL):
        dv = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib().vx_multi_create(mesh.h, dv, len(devices), kind, C.byref(h)))
        self.h = h
        self.n = len(devices)

    def voxelize(self, voxel_size, sat_variant=0, materials=False, all_gather=False):
        o = VoxelizeOpts()
        o.sat_variant = sat_variant
        o.flags = VOXELIZE_MATERIALS if materials else 0
        _check(lib().vx_multi_voxelize(self.h, np.float32(voxel_size), C.byref(o), 1 if all_gather else 0))
        return [BorrowedGrid(C.c_void_p(lib().vx_multi_grid(self.h, k))) for k in range(self.n if all_gather else 1)]


class Octree(_Handle):
    """vx_octree handle (the reference's Octree)."""
    _free = "vx_octree_free"

    def __init__(self, mesh, voxel_size, max_items=16, stream=None):
        h = C.c_void_p()
        _check(lib().vx_octree_build(mesh.h, np.float32(voxel_size), max_items, stream, C.byref(h)))
        self.h = h

    @property
    def num_items(self):
        return int(lib().vx_octree_num_items(self.h))

    @property
    def num_nodes(self):
        return int(lib().vx_octree_num_nodes(self.h))

    def memory_bytes(self):
        return int(lib().vx_octree_bytes(self.h))

    def items(self):
        n = self.num_items
        out = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib().vx_octree_items(self.h, out.ctypes.data, n))
        return out[:n]

    def nodes(self):
        n = self.num_nodes
        out = np.zeros(max(n, 1), dtype=NODE)
        _check(lib().vx_octree_nodes(self.h, out.ctypes.data, n))
        return out[:n]

    def root_bounds(self):
        mn, mx = (C.c_float * 3)(), (C.c_float * 3)()
        _check(lib().vx_octree_root_bounds(self.h, mn, mx))
        return np.array(mn, np.float32), np.array(mx, np.float32)

    def aabbs(self):
        n = C.c_uint64()
        _check(lib().vx_octree_aabbs(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=AABB)
        if n.value:
            _check(lib().vx_octree_aabbs(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def trace(self, rays, tmin=0.001, tmax=10000.0, want_prim=True):
        """vx_octree_trace: first hit per ray over the aabbs() list -> (t, prim, num_hits), or (t, num_hits) without prim."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        t = np.zeros(r.shape[0], dtype=np.float32)
        p = np.zeros(r.shape[0], dtype=np.uint32) if want_prim else None
        nh = C.c_uint64()
        _check(lib().vx_octree_trace(self.h, r.ctypes.data, r.shape[0], np.float32(tmin), np.float32(tmax), t.ctypes.data,
                                     p.ctypes.data if want_prim else None, C.byref(nh)))
        return (t, p, nh.value) if want_prim else (t, nh.value)

    def trace_ex(self, rays=None, camera=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, any_hit=False, want=("t", "prim")):
        """vx_octree_trace_ex: host-buffer extended query -> dict of the requested outputs (t, prim, normal, shadowed)."""
        return _trace_ex(lib().vx_octree_trace_ex, self.h, TraceArgs(), rays, camera, tmin, tmax, tmax_per_ray, any_hit, want)

    def trace_device(self, rays_ptr, nrays, t_ptr=None, prim_ptr=None, hits_ptr=None, nhits_ptr=None, tmin=0.001, tmax=10000.0,
                     normal_ptr=None, shadowed_ptr=None, tmax_per_ray_ptr=None, any_hit=False, camera=None):
        """vx_octree_trace_ex_device on device pointers (e.g. torch tensors' data_ptr()); camera = (view_inv, proj_inv, W, H) instead of rays."""
        _trace_ex_device(lib().vx_octree_trace_ex_device, self.h, TraceArgs(), rays_ptr, nrays, camera, tmin, tmax, any_hit, t=t_ptr, prim=prim_ptr,
                         normal=normal_ptr, shadowed=shadowed_ptr, tmax_per_ray=tmax_per_ray_ptr, hits=hits_ptr, num_hits=nhits_ptr)

    def trace_multi(self, rays=None, camera=None, max_hits=8, tmin=0.001, tmax=10000.0, tmax_per_ray=None, after=None, want=("t", "prim", "count")):
        """vx_octree_trace_multi on host arrays: per ray the first max_hits accepted voxels in (t, prim) order and the number of all of them
        -> dict as Grid.trace_multi gives it.  A voxel is a run of equal codes of the aabbs() list, prim the first list index of its run."""
        return _trace_multi(lib().vx_octree_trace_multi, self.h, MultiHitArgs(), 2, rays, camera, max_hits, tmin, tmax, tmax_per_ray, after, want)

    def trace_multi_device(self, rays_ptr, nrays, max_hits, t_ptr=None, prim_ptr=None, count_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None,
                           after_t_ptr=None, after_prim_ptr=None, camera=None):
        """vx_octree_trace_multi_device on raw device pointers, asynchronous on the octree's stream; t / prim hold max_hits entries per ray.
        camera = (view_inv, proj_inv, width, height) in place of rays_ptr / nrays."""
        _trace_multi_device(lib().vx_octree_trace_multi_device, self.h, MultiHitArgs(), rays_ptr, nrays, camera, max_hits, tmin, tmax, t=t_ptr,
                            prim=prim_ptr, count=count_ptr, tmax_per_ray=tmax_per_ray_ptr, after_t=after_t_ptr, after_prim=after_prim_ptr)


class Bvh(_Handle):
    """vx_bvh handle: the mesh's triangle BVH (the reference's triangle BLAS)."""
    _free = "vx_bvh_free"

    def __init__(self, mesh, max_leaf=0, stream=None):
        h = C.c_void_p()
        _check(lib().vx_bvh_build(mesh.h, max_leaf, stream, C.byref(h)))
        self.h = h

    def build_into(self, mesh):
        """vx_bvh_build_into: rebuild from the (refreshed) mesh in this handle's memory."""
        _check(lib().vx_bvh_build_into(mesh.h, self.h))

    @property
    def num_triangles(self):
        return int(lib().vx_bvh_num_triangles(self.h))

    @property
    def num_nodes(self):
        return int(lib().vx_bvh_num_nodes(self.h))

    @property
    def height(self):
        return int(lib().vx_bvh_height(self.h))

    @property
    def num_ill_conditioned(self):
        """triangles on the side list every ray tests (slivers, collinear)"""
        return int(lib().vx_bvh_num_ill_conditioned(self.h))

    def memory_bytes(self):
        return int(lib().vx_bvh_bytes(self.h))

    def nodes_device_ptr(self):
        return lib().vx_bvh_nodes_device(self.h)

    def nodes(self):
        """The node array decoded as BVH_NODE records (root at 0; leaf iff b & BVH_LEAF)."""
        nb = C.c_uint64()
        _check(lib().vx_bvh_nodes(self.h, None, 0, C.byref(nb)))
        out = np.zeros(max(nb.value // BVH_NODE.itemsize, 1), dtype=BVH_NODE)
        if nb.value:
            _check(lib().vx_bvh_nodes(self.h, out.ctypes.data, nb.value, C.byref(nb)))
        return out[:nb.value // BVH_NODE.itemsize]

    def leaf_triangles(self):
        """Triangle index of every leaf-order position."""
        n = self.num_triangles
        out = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().vx_bvh_leaf_triangles(self.h, out.ctypes.data, n))
        return out[:n]

    def root_bounds(self):
        mn, mx = (C.c_float * 3)(), (C.c_float * 3)()
        _check(lib().vx_bvh_root_bounds(self.h, mn, mx))
        return np.array(mn, np.float32), np.array(mx, np.float32)

    def trace(self, rays, tmin=0.001, tmax=10000.0, want_prim=True):
        """vx_bvh_trace: first hit per ray -> (t, prim, num_hits), or (t, num_hits) without prim."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        t = np.zeros(r.shape[0], dtype=np.float32)
        p = np.zeros(r.shape[0], dtype=np.uint32) if want_prim else None
        nh = C.c_uint64()
        _check(lib().vx_bvh_trace(self.h, r.ctypes.data, r.shape[0], np.float32(tmin), np.float32(tmax), t.ctypes.data,
                                  p.ctypes.data if want_prim else None, C.byref(nh)))
        return (t, p, nh.value) if want_prim else (t, nh.value)

    def trace_ex(self, rays=None, camera=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, any_hit=False, want=("t", "prim")):
        """vx_bvh_trace_ex: host-buffer extended query -> dict of the requested outputs (t, prim, normal, shadowed, bary)."""
        return _trace_ex(lib().vx_bvh_trace_ex, self.h, BvhTraceArgs(), rays, camera, tmin, tmax, tmax_per_ray, any_hit, want)

    def trace_device(self, rays_ptr, nrays, t_ptr=None, prim_ptr=None, hits_ptr=None, nhits_ptr=None, tmin=0.001, tmax=10000.0,
                     normal_ptr=None, shadowed_ptr=None, tmax_per_ray_ptr=None, any_hit=False, camera=None, bary_ptr=None):
        """vx_bvh_trace_ex_device on device pointers; camera = (view_inv, proj_inv, W, H) instead of rays."""
        _trace_ex_device(lib().vx_bvh_trace_ex_device, self.h, BvhTraceArgs(), rays_ptr, nrays, camera, tmin, tmax, any_hit, t=t_ptr, prim=prim_ptr,
                         normal=normal_ptr, shadowed=shadowed_ptr, tmax_per_ray=tmax_per_ray_ptr, hits=hits_ptr, num_hits=nhits_ptr, bary=bary_ptr)

    def trace_multi(self, rays=None, camera=None, max_hits=8, tmin=0.001, tmax=10000.0, tmax_per_ray=None, after=None, want=("t", "prim", "count")):
        """vx_bvh_trace_multi on host arrays: per ray the first max_hits accepted triangles in (t, prim) order and the number of all of them
        -> dict of the requested outputs (t, prim, bary, count).  after = (after_t, after_prim): per-ray cursor, only hits strictly behind it
        are listed and counted."""
        return _trace_multi(lib().vx_bvh_trace_multi, self.h, BvhMultiHitArgs(), 2, rays, camera, max_hits, tmin, tmax, tmax_per_ray, after, want)

    def trace_multi_device(self, rays_ptr, nrays, max_hits, t_ptr=None, prim_ptr=None, count_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None,
                           after_t_ptr=None, after_prim_ptr=None, camera=None, bary_ptr=None):
        """vx_bvh_trace_multi_device on raw device pointers, asynchronous on the BVH's stream; t / prim / bary hold max_hits entries per ray.
        camera = (view_inv, proj_inv, width, height) in place of rays_ptr / nrays."""
        _trace_multi_device(lib().vx_bvh_trace_multi_device, self.h, BvhMultiHitArgs(), rays_ptr, nrays, camera, max_hits, tmin, tmax, t=t_ptr,
                            prim=prim_ptr, count=count_ptr, tmax_per_ray=tmax_per_ray_ptr, after_t=after_t_ptr, after_prim=after_prim_ptr, bary=bary_ptr)


def instances(transforms, blas=None, mask=None):
    """(transforms[n, 12], blas[n], mask[n]) -> an INSTANCE array (blas defaults to 0, mask to 0xFF)."""
    tr = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
    out = np.zeros(tr.shape[0], dtype=INSTANCE)
    out["transform"] = tr
    out["blas"] = 0 if blas is None else np.asarray(blas, dtype=np.uint32)
    out["mask"] = 0xFF if mask is None else np.asarray(mask, dtype=np.uint32)
    return out


def _as_instances(inst):
    if isinstance(inst, np.ndarray) and inst.dtype == INSTANCE:
        return np.ascontiguousarray(inst)
    if isinstance(inst, tuple):
        return instances(*inst)
    return np.ascontiguousarray(np.asarray(inst), dtype=INSTANCE)


class Tlas(_Handle):
    """vx_tlas handle: a top-level structure over transformed instances of Bvh handles (borrowed: keep them alive)."""
    _free = "vx_tlas_free"

    def __init__(self, blas_list, instances, stream=None):
        self.blas = list(blas_list)
        inst = _as_instances(instances)
        arr = (C.c_void_p * max(len(self.blas), 1))(*[b.h for b in self.blas])
        h = C.c_void_p()
        _check(lib().vx_tlas_build(arr if self.blas else None, len(self.blas), inst.ctypes.data if len(inst) else None, len(inst),
                                   _stream_handle(stream), C.byref(h)))
        self.h = h

    def update(self, instances=None, device_ptr=None, count=None):
        """vx_tlas_update from host instances, or vx_tlas_update_device from a device array (a torch tensor of INSTANCE.itemsize-byte
        records, or a raw pointer with `count`)."""
        if device_ptr is not None:
            if hasattr(device_ptr, "data_ptr"):
                n = device_ptr.numel() * device_ptr.element_size() // INSTANCE.itemsize if count is None else count
                _check(lib().vx_tlas_update_device(self.h, device_ptr.data_ptr(), n))
            else:
                _check(lib().vx_tlas_update_device(self.h, device_ptr, count))
            return
        inst = _as_instances(instances)
        _check(lib().vx_tlas_update(self.h, inst.ctypes.data if len(inst) else None, len(inst)))

    def num_instances(self):
        return int(lib().vx_tlas_num_instances(self.h))

    def num_nodes(self):
        return int(lib().vx_tlas_num_nodes(self.h))

    def height(self):
        return int(lib().vx_tlas_height(self.h))

    def memory_bytes(self):
        return int(lib().vx_tlas_bytes(self.h))

    def world_to_object(self):
        n = self.num_instances()
        out = np.zeros((max(n, 1), 12), dtype=np.float32)
        _check(lib().vx_tlas_world_to_object(self.h, out.ctypes.data, n * 12))
        return out[:n]

    def nodes(self):
        nb = C.c_uint64()
        _check(lib().vx_tlas_nodes(self.h, None, 0, C.byref(nb)))
        out = np.zeros(max(nb.value // BVH_NODE.itemsize, 1), dtype=BVH_NODE)
        if nb.value:
            _check(lib().vx_tlas_nodes(self.h, out.ctypes.data, nb.value, C.byref(nb)))
        return out[:nb.value // BVH_NODE.itemsize]

    def trace(self, rays, tmin=0.001, tmax=10000.0):
        """vx_tlas_trace: first hit per ray -> (t, instance, prim, num_hits)."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        t = np.zeros(n, dtype=np.float32)
        ins = np.zeros(n, dtype=np.uint32)
        p = np.zeros(n, dtype=np.uint32)
        nh = C.c_uint64()
        _check(lib().vx_tlas_trace(self.h, r.ctypes.data, n, np.float32(tmin), np.float32(tmax), t.ctypes.data, ins.ctypes.data, p.ctypes.data,
                                   C.byref(nh)))
        return t, ins, p, nh.value

    def trace_ex(self, rays=None, camera=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, any_hit=False,
                 want=("t", "instance", "prim", "bary", "normal")):
        """vx_tlas_trace_ex: host-buffer query -> dict of the requested outputs (t, instance, prim, bary, normal, shadowed)."""
        return _trace_ex(lib().vx_tlas_trace_ex, self.h, TlasTraceArgs(), rays if camera is None else None, camera, tmin, tmax, tmax_per_ray, any_hit, want)

    def trace_device(self, rays_ptr, nrays, t_ptr=None, prim_ptr=None, instance_ptr=None, bary_ptr=None, normal_ptr=None, shadowed_ptr=None,
                     hits_ptr=None, nhits_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None, any_hit=False):
        """vx_tlas_trace_ex_device on device pointers."""
        _trace_ex_device(lib().vx_tlas_trace_ex_device, self.h, TlasTraceArgs(), rays_ptr, nrays, None, tmin, tmax, any_hit, t=t_ptr, prim=prim_ptr,
                         normal=normal_ptr, shadowed=shadowed_ptr, tmax_per_ray=tmax_per_ray_ptr, hits=hits_ptr, num_hits=nhits_ptr, bary=bary_ptr,
                         instance=instance_ptr)

    def trace_multi(self, rays=None, camera=None, max_hits=8, tmin=0.001, tmax=10000.0, tmax_per_ray=None, after=None, want=("t", "instance", "prim", "count")):
        """vx_tlas_trace_multi on host arrays: per ray the first max_hits accepted (instance, triangle) pairs in (t, instance, prim) order and
        the number of all of them -> dict of the requested outputs (t, instance, prim, bary, count).  after = (after_t, after_instance,
        after_prim): per-ray cursor."""
        return _trace_multi(lib().vx_tlas_trace_multi, self.h, TlasMultiHitArgs(), 3, rays, camera, max_hits, tmin, tmax, tmax_per_ray, after, want)

    def trace_multi_device(self, rays_ptr, nrays, max_hits, t_ptr=None, prim_ptr=None, count_ptr=None, tmin=0.001, tmax=10000.0, tmax_per_ray_ptr=None,
                           after_t_ptr=None, after_prim_ptr=None, camera=None, bary_ptr=None, instance_ptr=None, after_instance_ptr=None):
        """vx_tlas_trace_multi_device on raw device pointers, asynchronous on the TLAS's stream."""
        _trace_multi_device(lib().vx_tlas_trace_multi_device, self.h, TlasMultiHitArgs(), rays_ptr, nrays, camera, max_hits, tmin, tmax, t=t_ptr,
                            prim=prim_ptr, count=count_ptr, tmax_per_ray=tmax_per_ray_ptr, after_t=after_t_ptr, after_prim=after_prim_ptr, bary=bary_ptr,
                            instance=instance_ptr, after_instance=after_instance_ptr)


def _stream_handle(stream):
    """a torch.cuda.Stream, a raw hipStream_t (int) or None (the default stream) -> the pointer the C ABI takes"""
    if stream is None:
        return None
    return getattr(stream, "cuda_stream", stream)


class Renderer(_Handle):
    """vx_render_scene: whole frames on the device -- primary rays on the voxels (a Grid of kind GRID_BOOL, or an Octree) and the optional
    triangle model (bvh + the mesh it was built from), shadow rays, shading, gamma.  The scene borrows voxels, bvh and mesh: keep them
    alive while it is in use (this object holds references to them)."""
    _free = "vx_render_free"

    def __init__(self, voxels, bvh=None, mesh=None, stream=None, attributes=False):
        d = RenderDesc()
        if isinstance(voxels, Octree):
            d.octree = voxels.h
        else:
            d.grid = voxels.h
        d.bvh = bvh.h if bvh is not None else None
        d.mesh = mesh.h if mesh is not None else None
        self._create(lib().vx_render_create, d, (voxels, bvh, mesh), stream, attributes)

    def _create(self, create, desc, keep, stream, attributes):
        """what both constructors end with: the scene of `desc` on `stream`, the objects it borrows kept alive, the shading flag applied"""
        desc.stream = _stream_handle(stream)
        self._torch_stream = stream if hasattr(stream, "cuda_stream") else None
        self._keep = keep
        h = C.c_void_p()
        _check(create(C.byref(desc), C.byref(h)))
        self.h = h
        if attributes:
            self.set_shading(RENDER_ATTRIBUTES)

    @classmethod
    def from_tlas(cls, voxels=None, tlas=None, meshes=(), stream=None, attributes=False):
        """vx_render_create_tlas: an instanced scene -- at most one voxel source (Grid of kind GRID_BOOL, Octree or None), a Tlas and one
        Mesh per BLAS of it (vertices, indices, materials), in the Tlas's BLAS order."""
        self = cls.__new__(cls)
        d = RenderTlasDesc()
        if isinstance(voxels, Octree):
            d.octree = voxels.h
        elif voxels is not None:
            d.grid = voxels.h
        d.tlas = tlas.h if tlas is not None else None
        meshes = list(meshes)
        arr = (C.c_void_p * max(len(meshes), 1))(*[m.h if m is not None else None for m in meshes])
        d.meshes = C.cast(arr, C.c_void_p) if meshes else None
        self._create(lib().vx_render_create_tlas, d, (voxels, tlas, meshes), stream, attributes)
        return self

    def set_shading(self, flags):
        """vx_render_set_shading: RENDER_ATTRIBUTES (corner normals and diffuse textures of triangle hits) or 0, from the next frame"""
        _check(lib().vx_render_set_shading(self.h, int(flags)))

    @staticmethod
    def _args(camera, light):
        vi, pi, w, h = camera
        a = RenderArgs()
        cvi = (C.c_float * 16)(*[float(x) for x in np.asarray(vi, np.float32).reshape(16)])
        cpi = (C.c_float * 16)(*[float(x) for x in np.asarray(pi, np.float32).reshape(16)])
        a.view_inverse, a.proj_inverse, a.width, a.height = cvi, cpi, int(w), int(h)
        keep = [cvi, cpi]
        if light is not None:
            pos, intensity, kind = light
            lt = RenderLight()
            lt.position = (C.c_float * 3)(*[float(x) for x in np.asarray(pos, np.float32).reshape(3)])
            lt.intensity, lt.type = float(np.float32(intensity)), int(kind)
            a.light = C.pointer(lt)
            keep.append(lt)
        return a, keep

    def render(self, camera, light=None, out=None, kind=None, shadowed=None):
        """vx_render_frame_device, asynchronous on the scene's stream -> `out`, a device torch.uint8 tensor [H, W, 4] (RGBA8).
        camera = (view_inv, proj_inv, W, H) as for trace_ex; light = (position[3], intensity, type 0 point / 1 directional), None = the
        reference's default point light; kind / shadowed: optional device uint8 tensors of H*W elements."""
        import torch
        w, h = int(camera[2]), int(camera[3])
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        if out.dtype != torch.uint8 or out.numel() != 4 * w * h or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("out must be a contiguous device uint8 tensor of H*W*4 elements")
        for x in (kind, shadowed):
            if x is not None and (x.dtype != torch.uint8 or x.numel() != w * h or not x.is_contiguous() or not x.is_cuda):
                raise ValueError("kind / shadowed must be contiguous device uint8 tensors of H*W elements")
        a, keep = self._args(camera, light)
        a.rgba = out.data_ptr()
        a.kind = kind.data_ptr() if kind is not None else None
        a.shadowed = shadowed.data_ptr() if shadowed is not None else None
        _check(lib().vx_render_frame_device(self.h, C.byref(a)))
        if self._torch_stream is not None:  # the caching allocator must not hand these out again before the frame has written them
            for x in (out, kind, shadowed):
                if x is not None:
                    x.record_stream(self._torch_stream)
        return out

    def render_host(self, camera, light=None, want=("rgba",)):
        """vx_render_frame on host buffers -> dict: rgba uint8[H, W, 4], and on request kind / shadowed uint8[H, W]."""
        w, h = int(camera[2]), int(camera[3])
        a, keep = self._args(camera, light)
        out = {"rgba": np.zeros((h, w, 4), np.uint8)}
        a.rgba = out["rgba"].ctypes.data
        for k in ("kind", "shadowed"):
            if k in want:
                out[k] = np.zeros((h, w), np.uint8)
                setattr(a, k, out[k].ctypes.data)
        _check(lib().vx_render_frame(self.h, C.byref(a)))
        return out

    def refresh(self):
        """vx_render_refresh: re-read the material and attribute tables (corner attributes, textures) of the sources."""
        _check(lib().vx_render_refresh(self.h))

    def free(self):
        super().free()
        self._keep = None
