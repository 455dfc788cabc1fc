"""CPU tests of the instanced scenes (vx_tlas_*): the entry points are exported and listed in voxhip.SYMBOLS, every argument error is
reported before any device work, VX_ERR_NO_DEVICE where there is no device, and the numpy restatement of the contract
(tests/instance_ref.py) behaves as include/voxhip.h pins it on hand-worked cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_ref  # noqa: E402
import mesh_ref  # noqa: E402

INVALID_ARG, NO_DEVICE = 1, 6
TLAS_SYMBOLS = ("vx_tlas_build", "vx_tlas_update", "vx_tlas_update_device", "vx_tlas_num_instances", "vx_tlas_num_nodes", "vx_tlas_height",
                "vx_tlas_bytes", "vx_tlas_world_to_object", "vx_tlas_nodes", "vx_tlas_trace_ex_device", "vx_tlas_trace_ex", "vx_tlas_trace",
                "vx_tlas_free")
IDENT = instance_ref.transform()
SQ_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
SQ_T = np.int32([[0, 1, 2], [1, 3, 2]])


def rays(*pairs):
    return np.float32([list(o) + list(d) for o, d in pairs])


def test_tlas_symbols_exported(vx):
    L = C.CDLL(vx.LIB_PATH)
    for n in TLAS_SYMBOLS:
        assert hasattr(L, n) and n in vx.SYMBOLS, n
    for m in ("update", "world_to_object", "nodes", "height", "num_instances", "memory_bytes", "trace", "trace_ex", "trace_device", "free"):
        assert hasattr(vx.Tlas, m), m
    assert vx.INSTANCE.itemsize == 56 and vx.INSTANCE == instance_ref.INSTANCE


def test_tlas_argument_errors_before_device_work(vx):
    L = vx.lib()
    h = C.c_void_p()
    fake = C.create_string_buffer(4096)                 # a non-null handle the checks must never dereference
    arr = (C.c_void_p * 1)(C.addressof(fake))
    nul = (C.c_void_p * 1)(None)
    inst = instance_ref.make_instances([IDENT])
    ip = inst.ctypes.data
    assert L.vx_tlas_build(None, 0, None, 0, None, None) == INVALID_ARG                 # no out
    assert L.vx_tlas_build(None, 1, ip, 1, None, C.byref(h)) == INVALID_ARG             # num_blas without a list
    assert L.vx_tlas_build(nul, 1, ip, 1, None, C.byref(h)) == INVALID_ARG              # a null BLAS handle
    assert L.vx_tlas_build(None, 0, ip, 1, None, C.byref(h)) == INVALID_ARG             # instances without BLAS
    assert L.vx_tlas_build(arr, 1, None, 1, None, C.byref(h)) == INVALID_ARG            # null instances
    bad = instance_ref.make_instances([IDENT], blas=[1])
    assert L.vx_tlas_build(arr, 1, bad.ctypes.data, 1, None, C.byref(h)) == INVALID_ARG
    assert b"blas index" in L.vx_last_error()
    for v in (np.nan, np.inf, -np.inf):
        nf = instance_ref.make_instances([IDENT])
        nf["transform"][0, 7] = v
        assert L.vx_tlas_build(arr, 1, nf.ctypes.data, 1, None, C.byref(h)) == INVALID_ARG
        assert b"non-finite" in L.vx_last_error()
    assert not h.value
    assert L.vx_tlas_update(None, ip, 1) == INVALID_ARG
    assert L.vx_tlas_update_device(None, ip, 1) == INVALID_ARG
    t = np.zeros(1, np.float32)
    r = np.zeros((1, 6), np.float32)
    assert L.vx_tlas_trace(None, r.ctypes.data, 1, np.float32(0.001), np.float32(1e4), t.ctypes.data, None, None, None) == INVALID_ARG
    a = vx.TlasTraceArgs()
    a.base.rays, a.base.num_rays, a.base.t = r.ctypes.data, 1, t.ctypes.data
    assert L.vx_tlas_trace_ex(None, C.byref(a)) == INVALID_ARG
    assert L.vx_tlas_trace_ex_device(None, C.byref(a)) == INVALID_ARG
    assert L.vx_tlas_world_to_object(None, None, 0) == INVALID_ARG
    assert L.vx_tlas_nodes(None, None, 0, None) == INVALID_ARG
    assert L.vx_tlas_num_instances(None) == 0 and L.vx_tlas_num_nodes(None) == 0 and L.vx_tlas_bytes(None) == 0 and L.vx_tlas_height(None) == 0
    L.vx_tlas_free(None)


def test_tlas_no_device(vx):
    if vx.device_count() > 0:
        pytest.skip("a HIP device is present")
    h = C.c_void_p()
    assert vx.lib().vx_tlas_build(None, 0, None, 0, None, C.byref(h)) == NO_DEVICE   # valid arguments, no device: no CPU path
    assert not h.value


def test_ref_identity_equals_mesh_ref():
    rng = np.random.default_rng(1)
    r = np.concatenate([rng.uniform(-1, 2, (300, 3)), rng.standard_normal((300, 3))], axis=1).astype(np.float32)
    r[:100, 2] = 1.0
    r[:100, 3:] = [0, 0, -1]
    t0, p0, b0 = mesh_ref.closest(SQ_V, SQ_T, r)
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], instance_ref.make_instances([IDENT]), r)
    assert np.array_equal(t, t0) and np.array_equal(p, p0) and np.array_equal(b, b0)
    assert np.array_equal(i, np.where(t > 0, 0, instance_ref.MISS).astype(np.uint32))
    w, det = instance_ref.inverse([IDENT])
    assert det[0] == 1.0 and np.array_equal(w[0], IDENT)


def test_ref_translated_instance():
    inst = instance_ref.make_instances([instance_ref.transform(offset=(10, 0, 0))])
    r = rays(((10.25, 0.25, 1), (0, 0, -1)), ((0.25, 0.25, 1), (0, 0, -1)))
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], inst, r)
    assert t[0] == 1.0 and i[0] == 0 and p[0] == 0 and np.array_equal(b[0], [0.25, 0.25])
    assert t[1] == -1 and i[1] == instance_ref.MISS and p[1] == instance_ref.MISS
    w, _ = instance_ref.inverse(inst["transform"])
    assert np.array_equal(w[0], instance_ref.transform(offset=(-10, 0, 0)))
    assert np.array_equal(instance_ref.world_normals([(SQ_V, SQ_T)], inst, i, p)[0], [0, 0, 1])


def test_ref_mirrored_and_scaled_instances():
    # mirror in x (det < 0): the square covers x in [-1, 0]; the world normal keeps cross(e1, e2) of the MIRRORED triangle: (0, 0, -1)
    inst = instance_ref.make_instances([instance_ref.transform(scale=(-1, 1, 1))])
    r = rays(((-0.25, 0.25, 1), (0, 0, -1)), ((0.25, 0.25, 1), (0, 0, -1)))
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], inst, r)
    assert t[0] == 1.0 and p[0] == 0 and t[1] == -1
    assert np.array_equal(instance_ref.world_normals([(SQ_V, SQ_T)], inst, i, p)[0], [0, 0, -1])
    _, det = instance_ref.inverse(inst["transform"])
    assert det[0] == -1.0
    # non-uniform scale: x by 4, z by 2, lifted to z = 3; t is parametric in the world ray
    inst = instance_ref.make_instances([instance_ref.transform(scale=(4, 1, 2), offset=(0, 0, 3))])
    r = rays(((3.0, 0.5, 5), (0, 0, -1)), ((3.0, 0.5, 5), (0, 0, -0.5)), ((4.5, 0.1, 5), (0, 0, -1)))
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], inst, r)
    assert t[0] == 2.0 and t[1] == 4.0 and t[2] == -1
    assert p[0] == 1 and np.array_equal(b[0], [0.25, 0.25])   # (0.75, 0.5) in the square: the second triangle, v0 = (1, 0)
    assert np.array_equal(instance_ref.world_normals([(SQ_V, SQ_T)], inst, i, p)[0], [0, 0, 1])
    hp = instance_ref.world_hit_points([(SQ_V, SQ_T)], inst, i, p, b)
    assert np.allclose(hp[0], [3.0, 0.5, 3.0])


def test_ref_tie_between_identical_instances_picks_the_lower_index():
    inst = instance_ref.make_instances([instance_ref.transform(offset=(0, 0, 1)), IDENT, IDENT], mask=[0xFF, 0xFF, 0xFF])
    r = rays(((0.25, 0.25, 2), (0, 0, -1)), ((0.25, 0.25, -2), (0, 0, 1)))
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], inst, r)
    assert t[0] == 1.0 and i[0] == 0           # the lifted square first from above
    assert t[1] == 2.0 and i[1] == 1           # from below: instances 1 and 2 coincide; the lower index wins
    inst["mask"][1] = 0
    t, i, p, b = instance_ref.closest([(SQ_V, SQ_T)], inst, r)
    assert t[1] == 2.0 and i[1] == 2
    assert instance_ref.any_hit([(SQ_V, SQ_T)], inst, r).tolist() == [1, 1]


def test_ref_inactive_instances():
    sing = instance_ref.transform(scale=(1, 0, 1))
    inst = instance_ref.make_instances([sing, IDENT, IDENT], blas=[0, 1, 0], mask=[0xFF, 0xFF, 0])
    meshes = [(SQ_V, SQ_T), (SQ_V, np.zeros((0, 3), np.int32))]
    assert instance_ref.active(inst, [2, 0]).tolist() == [False, False, False]
    t, i, p, b = instance_ref.closest(meshes, inst, rays(((0.25, 0.25, 1), (0, 0, -1))))
    assert t[0] == -1 and i[0] == instance_ref.MISS


def test_ref_pinned_inverse_agrees_with_numpy_linalg():
    rng = np.random.default_rng(5)
    tr = []
    for _ in range(200):
        rot = instance_ref.random_rotation(rng)
        tr.append(instance_ref.transform(rot, rng.uniform(0.2, 5, 3) * rng.choice([-1, 1], 3), rng.uniform(-0.5, 0.5), rng.uniform(-100, 100, 3)))
    tr = np.asarray(tr, np.float32)
    w, det = instance_ref.inverse(tr)
    for k in range(len(tr)):
        a = np.zeros((4, 4))
        a[:3] = tr[k].reshape(3, 4).astype(np.float64)
        a[3, 3] = 1
        inv = np.linalg.inv(a)[:3].reshape(12).astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(inv), np.abs(w[k]).max() * 2.0 ** -12).astype(np.float32))
        assert (np.abs(w[k] - inv) <= 4 * ulp).all(), (k, w[k], inv)
        assert np.isclose(det[k], np.linalg.det(a[:3, :3]), rtol=1e-12)
