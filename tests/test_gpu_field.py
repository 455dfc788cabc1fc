"""GPU tests of the distance-field queries (vx_field: vx_field_sample*, vx_field_sphere_trace*): every output is compared bit for bit with
the restatement (tests/field_ref.py) evaluated on the GPU's own sdf() of the same grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import field_cases as fc
import field_ref as fr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
DIMS = [(1, 1, 1), (2, 1, 3), (33, 1, 7), (5, 4, 3), (97, 45, 31)]
DENSITIES = [0.0, 0.01, 0.5, 1.0]
PATTERN = 0xA5


def masked_grid(gpu, cells, vs):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, Z, vs, fc.ORG)
    write_mask(g, dr.pack(cells))
    g.refresh()
    return g


def random_cells(dims, density):
    X, Y, Z = dims
    return np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density


def geometry(g):
    d = g.describe()
    return g.sdf(), tuple(float(x) for x in d["origin"]), F(d["voxel_size"]), d["dim"]


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d bytes differ" % (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()))


def all_points(dims, org, vs):
    return np.concatenate([fc.cell_centres(dims, org, vs), fc.edge_points(dims, org, vs), fc.random_points(dims, org, vs, 4096, 1)])


def check_sample(f, S, org, vs, pts, alone=False):
    v, g, o = fr.sample(S, org, vs, pts)
    got = f.sample(pts)
    same_bits(got["value"], v, "value")
    same_bits(got["gradient"], g, "gradient")
    same_bits(got["occupied"], o, "occupied")
    if alone:
        for name, ref in (("value", v), ("gradient", g), ("occupied", o)):
            one = f.sample(pts, want=(name,))
            assert list(one) == [name]
            same_bits(one[name], ref, name + " alone")
    return v, g, o


def check_trace(f, S, org, vs, rays, **kw):
    t, c, s, st = fr.sphere_trace(S, org, vs, rays, **kw)
    got = f.sphere_trace(rays, **kw)
    same_bits(got["status"], st, "status")
    same_bits(got["steps"], s, "steps")
    same_bits(got["t"], t, "t")
    same_bits(got["clearance"], c, "clearance")
    return t, c, s, st


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("density", DENSITIES)
def test_random_masks(gpu, dims, density):
    cells = random_cells(dims, density)
    for vs in (fc.VS_ODD, fc.VS_DYADIC):
        g = masked_grid(gpu, cells, vs)
        S, org, vs_, d = geometry(g)
        f = g.field()
        desc = f.describe()
        assert desc["dim"] == dims and desc["voxel_size"] == float(vs) and desc["bytes"] == 4 * cells.size
        assert desc["state"] == (gpu.FIELD_EMPTY if not cells.any() else gpu.FIELD_FULL if cells.all() else gpu.FIELD_FINITE)
        v, gr, o = check_sample(f, S, org, vs, all_points(dims, org, vs), alone=dims == (5, 4, 3))
        n = cells.size
        if vs == fc.VS_DYADIC and desc["state"] == gpu.FIELD_FINITE:
            same_bits(v[:n], S.reshape(-1), "the cell centres of a dyadic geometry")
        assert np.array_equal(o[:n], cells.reshape(-1).astype(np.uint8))
        assert np.abs(gr).max() <= 2.0 * (1 + 4 * 2.0 ** -23)
        rays = np.concatenate([fc.random_rays(dims, org, vs, 1024, 2), fc.special_rays(cells | ~cells.any(), org, vs)])
        for radius in (0.0, float(F(2.3) * vs)):
            t, c, s, st = check_trace(f, S, org, vs, rays, radius=radius)
            if desc["state"] == gpu.FIELD_EMPTY:
                assert (st == fr.MISS).all() and (t == -1).all()
            if desc["state"] == gpu.FIELD_FULL:
                inside = min(16, cells.size)  # (special_rays starts with rays from inside occupied cells)
                assert (st[1024:1024 + inside] == fr.HIT).all() and (c[st == fr.HIT] == -np.inf).all()
        f.free()
        g.free()


@pytest.fixture(scope="module")
def proto(gpu):
    """the ball, plate and noise on 40 x 36 x 31 at vs 0.37: grid, field, S, origin, vs, dims, 4096 random rays"""
    dims = (40, 36, 31)
    cells = fc.prototype_mask(dims)
    g = masked_grid(gpu, cells, fc.VS_ODD)
    S, org, vs, d = geometry(g)
    f = g.field()
    return dict(g=g, f=f, S=S, org=org, vs=vs, dims=dims, cells=cells, rays=fc.random_rays(dims, org, vs, 4096, 7))


@pytest.mark.parametrize("radius_cells", [0.0, 2.3])
def test_random_rays_hit_and_miss(gpu, proto, radius_cells):
    p = proto
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], p["rays"], radius=float(F(radius_cells) * p["vs"]))
    assert (st == fr.HIT).mean() >= 0.1 and (st == fr.MISS).mean() >= 0.1, np.bincount(st, minlength=3)
    assert (t[st == fr.HIT] >= 0).all() and (t[st != fr.HIT] == -1).all()


def test_rays_from_inside_hit_at_once(gpu, proto):
    p = proto
    rays = fc.special_rays(p["cells"], p["org"], p["vs"])[:16]
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], rays, tmin=0.0)
    assert (st == fr.HIT).all() and (t == 0).all() and (s == 1).all() and (c < 0).all()


def test_special_rays(gpu, proto):
    p = proto
    rays = fc.special_rays(p["cells"], p["org"], p["vs"])
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], rays)
    bad = ~np.isfinite(rays).all(axis=1)
    assert bad.sum() == 18 and (st[bad] == fr.MISS).all() and (s[bad] == 0).all() and np.isposinf(c[bad]).all()
    sa = s[16:40].reshape(6, 4)  # per axis and sign: through the middle, outside the slab, on its face, denormal components
    assert (sa[:, 0] > 0).all() and (sa[:, 1] == 0).all() and (sa[:, 2] > 0).all()


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scaled_directions(gpu, proto, scale):
    p = proto
    rays = p["rays"][:1024].copy()
    t1, _, _, st1 = fr.sphere_trace(p["S"], p["org"], p["vs"], rays)
    rays[:, 3:] *= F(scale)
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], rays, tmin=0.001 / scale, tmax=10000.0 / scale)
    both = (st == fr.HIT) & (st1 == fr.HIT)
    assert both.sum() > 100 and np.allclose(t[both] * scale, t1[both], rtol=1e-3, atol=1e-3)


def test_per_ray_radius_and_tmax(gpu, proto):
    p = proto
    rays = p["rays"][:1024]
    t0, _, _, st0 = fr.sphere_trace(p["S"], p["org"], p["vs"], rays)
    rng = np.random.default_rng(9)
    rpr = (rng.random(1024) * 3 * p["vs"]).astype(F)
    rpr[:3] = (-1.0, np.nan, np.inf)
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], rays, radius=123.0, radius_per_ray=rpr)
    assert (st[:3] == fr.MISS).all() and (s[:3] == 0).all()
    hit = st0 == fr.HIT
    tpr = np.where(hit, t0 * F(0.5), F(10000.0)).astype(F)   # cut before the hit
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], rays, tmax_per_ray=tpr)
    late = hit & (t0 * F(0.5) > F(0.01))
    assert late.sum() > 100 and (st[late & (s > 1)] != fr.HIT).any()


@pytest.mark.parametrize("max_steps", [1, 3])
def test_step_limit(gpu, proto, max_steps):
    p = proto
    t, c, s, st = check_trace(p["f"], p["S"], p["org"], p["vs"], p["rays"], max_steps=max_steps)
    assert (s <= max_steps).all()
    if max_steps == 3:
        assert (st == fr.STEP_LIMIT).mean() >= 0.5, np.bincount(st, minlength=3)


def test_march_parameters(gpu, proto):
    p = proto
    check_trace(p["f"], p["S"], p["org"], p["vs"], p["rays"][:1024], radius=float(F(1.1) * p["vs"]), step_scale=float(F(1.0 / (2 * np.sqrt(3.0)))), hit_eps=0.001,
                max_steps=65535)
    check_trace(p["f"], p["S"], p["org"], p["vs"], p["rays"][:1024], step_scale=1.0, hit_eps=0.5, tmin=2.0, tmax=6.0)
    # zeros ask for the defaults
    a = p["f"].sphere_trace(p["rays"][:256], step_scale=0.0, hit_eps=0.0, max_steps=0)
    b = p["f"].sphere_trace(p["rays"][:256])
    for k in a:
        same_bits(a[k], b[k], k)


def test_each_trace_output_alone(gpu, proto):
    p = proto
    full = p["f"].sphere_trace(p["rays"][:300])
    for name in ("t", "clearance", "steps", "status"):
        one = p["f"].sphere_trace(p["rays"][:300], want=(name,))
        assert list(one) == [name]
        same_bits(one[name], full[name], name)


def test_mesh_field_in_all_grid_kinds(gpu):
    v, t = vx_scenes.scene("rotcube")
    mesh = gpu.Mesh.from_arrays(v, t)
    first = None
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, F(0.09), kind)
        S, org, vs, dims = geometry(g)
        f = g.field()
        pts = np.concatenate([fc.edge_points(dims, org, vs), fc.random_points(dims, org, vs, 4096, 1)])
        rays = fc.random_rays(dims, org, vs, 2048, 2)
        res = check_sample(f, S, org, vs, pts) + check_trace(f, S, org, vs, rays, radius=0.05)
        if first is None:
            first = res
            assert (res[6] == fr.HIT).any() and (res[6] == fr.MISS).any()
        for a, b in zip(res, first):
            same_bits(a, b, "grid kinds")
        f.free()


# ---- handle behaviour ----------------------------------------------------------------------------------------------------------
def test_device_variants_equal_host_variants(gpu, proto):
    import torch
    p = proto
    f = p["f"]
    pts = all_points(p["dims"], p["org"], p["vs"])
    n = len(pts)
    dp = torch.from_numpy(pts).cuda()
    v = torch.empty(n, dtype=torch.float32, device="cuda")
    g = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    o = torch.empty(n, dtype=torch.uint8, device="cuda")
    f.sample_device(dp.data_ptr(), n, v.data_ptr(), g.data_ptr(), o.data_ptr())
    torch.cuda.synchronize()
    host = f.sample(pts)
    same_bits(v.cpu().numpy(), host["value"], "value")
    same_bits(g.cpu().numpy(), host["gradient"], "gradient")
    same_bits(o.cpu().numpy(), host["occupied"], "occupied")
    # the snapshot itself is sdf()'s values
    snap = torch.empty(p["S"].size, dtype=torch.float32, device="cuda")

    class View:
        __cuda_array_interface__ = {"shape": (p["S"].size,), "typestr": "<f4", "data": (f.values_device_ptr(), False), "version": 3, "strides": None}
    snap.copy_(torch.as_tensor(View(), device="cuda"))
    same_bits(snap.cpu().numpy(), p["S"].reshape(-1), "values_device")
    rays = p["rays"]
    m = len(rays)
    rpr = (np.random.default_rng(4).random(m) * 2 * p["vs"]).astype(F)
    tpr = (np.random.default_rng(5).random(m) * 30).astype(F)
    dr_, drp, dtp = torch.from_numpy(rays).cuda(), torch.from_numpy(rpr).cuda(), torch.from_numpy(tpr).cuda()
    t = torch.empty(m, dtype=torch.float32, device="cuda")
    c = torch.empty(m, dtype=torch.float32, device="cuda")
    s = torch.empty(m, dtype=torch.int32, device="cuda")
    st = torch.empty(m, dtype=torch.uint8, device="cuda")
    f.sphere_trace_device(dr_.data_ptr(), m, radius_per_ray_ptr=drp.data_ptr(), tmax_per_ray_ptr=dtp.data_ptr(), t_ptr=t.data_ptr(), clearance_ptr=c.data_ptr(),
                          steps_ptr=s.data_ptr(), status_ptr=st.data_ptr())
    torch.cuda.synchronize()
    host = f.sphere_trace(rays, radius_per_ray=rpr, tmax_per_ray=tpr)
    same_bits(t.cpu().numpy(), host["t"], "t")
    same_bits(c.cpu().numpy(), host["clearance"], "clearance")
    same_bits(s.cpu().numpy().view(np.uint32), host["steps"], "steps")
    same_bits(st.cpu().numpy(), host["status"], "status")
    rt, rc, rs, rst = fr.sphere_trace(p["S"], p["org"], p["vs"], rays, radius_per_ray=rpr, tmax_per_ray=tpr)
    same_bits(host["t"], rt, "t against the restatement")
    same_bits(host["status"], rst, "status against the restatement")


def test_update_equals_a_fresh_create_and_refuses_other_dimensions(gpu):
    dims = (33, 9, 7)
    a, b = random_cells(dims, 0.05), random_cells(dims, 0.5)
    g = masked_grid(gpu, a, fc.VS_ODD)
    f = g.field()
    write_mask(g, dr.pack(b))
    g.refresh()
    S, org, vs, d = geometry(g)
    n0 = gpu.device_allocations()
    f.update(g)
    assert gpu.device_allocations() == n0
    fresh = g.field()
    pts = all_points(dims, org, vs)
    rays = fc.random_rays(dims, org, vs, 1024, 2)
    r1 = check_sample(f, S, org, vs, pts) + check_trace(f, S, org, vs, rays)
    r2 = check_sample(fresh, S, org, vs, pts) + check_trace(fresh, S, org, vs, rays)
    for x, y in zip(r1, r2):
        same_bits(x, y, "update against create")
    other = masked_grid(gpu, random_cells((33, 9, 8), 0.5), fc.VS_ODD)
    with pytest.raises(gpu.VxError) as e:
        f.update(other)
    assert e.value.status == INVALID_ARG
    check_sample(f, S, org, vs, pts)  # (the refused update changed nothing)
    # an update to an empty and to a full mask takes the state anew
    for cells, state in ((np.zeros_like(a), gpu.FIELD_EMPTY), (np.ones_like(a), gpu.FIELD_FULL)):
        write_mask(g, dr.pack(cells))
        g.refresh()
        f.update(g)
        assert f.describe()["state"] == state
        check_sample(f, g.sdf(), org, vs, pts[-200:])


def test_queries_after_the_grid_is_freed(gpu):
    dims = (33, 9, 7)
    g = masked_grid(gpu, random_cells(dims, 0.1), fc.VS_ODD)
    S, org, vs, d = geometry(g)
    f = g.field()
    g.free()
    junk = masked_grid(gpu, random_cells((64, 64, 64), 0.5), fc.VS_DYADIC)  # (takes the freed grid's blocks from the pool)
    junk.sdf()
    check_sample(f, S, org, vs, all_points(dims, org, vs))
    check_trace(f, S, org, vs, fc.random_rays(dims, org, vs, 1024, 2))


def test_repeated_queries_allocate_nothing_and_free_returns_every_block(gpu, proto):
    p = proto
    g = masked_grid(gpu, p["cells"], fc.VS_ODD)
    g.sdf()
    live0 = gpu.device_live_blocks()
    f = g.field()
    assert gpu.device_live_blocks() > live0
    pts, rays = all_points(p["dims"], p["org"], p["vs"]), p["rays"]
    rpr = np.full(len(rays), 0.1, dtype=F)
    f.sample(pts)
    f.sphere_trace(rays, radius_per_ray=rpr, tmax_per_ray=rpr + 50)
    n0 = gpu.device_allocations()
    a = f.sample(pts)
    b = f.sphere_trace(rays, radius_per_ray=rpr, tmax_per_ray=rpr + 50)
    assert gpu.device_allocations() == n0
    same_bits(a["value"], fr.value(p["S"], p["org"], p["vs"], pts), "value")
    same_bits(b["status"], fr.sphere_trace(p["S"], p["org"], p["vs"], rays, radius_per_ray=rpr, tmax_per_ray=rpr + 50)[3], "status")
    f.free()
    assert gpu.device_live_blocks() == live0


def test_poisoned_pool_blocks_change_nothing(gpu, proto):
    p = proto
    pts, rays = all_points(p["dims"], p["org"], p["vs"]), p["rays"][:1024]
    gpu.pool_poison(0xA5A5A5A5)
    try:
        g = masked_grid(gpu, p["cells"], fc.VS_ODD)
        f = g.field()
        check_sample(f, p["S"], p["org"], p["vs"], pts, alone=True)
        check_trace(f, p["S"], p["org"], p["vs"], rays, radius=0.3)
        f.free()
        g.free()
    finally:
        gpu.pool_poison(None)


def test_create_checks(gpu):
    L = gpu.lib()
    g = masked_grid(gpu, random_cells((5, 4, 3), 0.5), fc.VS_ODD)
    h = C.c_void_p(0x1234)
    assert L.vx_field_create(None, None, C.byref(h)) == INVALID_ARG and h.value is None
    assert L.vx_field_create(g.h, None, None) == INVALID_ARG
    empty = gpu.Grid.create(gpu.GRID_BOOL, 0, 4, 3, F(0.5))
    h = C.c_void_p(0x1234)
    assert L.vx_field_create(empty.h, None, C.byref(h)) == INVALID_ARG and h.value is None
    long = gpu.Grid.create(gpu.GRID_BOOL, 65537, 1, 1, F(0.5))
    h = C.c_void_p(0x1234)
    assert L.vx_field_create(long.h, None, C.byref(h)) == CAPACITY and h.value is None
    with pytest.raises(gpu.VxError) as e:
        long.sdf()
    assert e.value.status == CAPACITY
    assert L.vx_field_update(None, g.h) == INVALID_ARG
    f = g.field()
    assert L.vx_field_update(f.h, None) == INVALID_ARG
    assert L.vx_field_describe(None, C.byref(gpu.FieldDesc())) == INVALID_ARG and L.vx_field_describe(f.h, None) == INVALID_ARG
    assert L.vx_field_values_device(None) is None
    L.vx_field_free(None)


def patterned(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, PATTERN, dtype=np.uint8).view(dtype)


def test_query_checks_write_nothing(gpu, proto):
    L, f = gpu.lib(), proto["f"]
    n = 64
    pts = np.ascontiguousarray(fc.random_points(proto["dims"], proto["org"], proto["vs"], n, 1))
    rays = np.ascontiguousarray(proto["rays"][:n])
    outs = dict(value=patterned(n, F), gradient=patterned(3 * n, F), occupied=patterned(n, np.uint8), t=patterned(n, F), clearance=patterned(n, F),
                steps=patterned(n, np.uint32), status=patterned(n, np.uint8))

    def untouched():
        return all((a.view(np.uint8) == PATTERN).all() for a in outs.values())

    def sample_args(points=pts.ctypes.data, num=n, names=("value", "gradient", "occupied")):
        a = gpu.FieldSampleArgs()
        a.points, a.num_points = points, num
        for k in names:
            setattr(a, k, outs[k].ctypes.data)
        return a

    def trace_args(rays_=rays.ctypes.data, num=n, names=("t", "clearance", "steps", "status"), **kw):
        a = gpu.FieldTraceArgs()
        a.rays, a.num_rays, a.tmin, a.tmax = rays_, num, 0.001, 10000.0
        for k in names:
            setattr(a, k, outs[k].ctypes.data)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn in (L.vx_field_sample, L.vx_field_sample_device):
        assert fn(None, C.byref(sample_args())) == INVALID_ARG
        assert fn(f.h, None) == INVALID_ARG
        assert fn(f.h, C.byref(sample_args(points=None))) == INVALID_ARG
        assert fn(f.h, C.byref(sample_args(names=()))) == INVALID_ARG
        assert fn(f.h, C.byref(sample_args(num=0))) == 0
        assert fn(f.h, C.byref(sample_args(points=None, num=0))) == 0
        assert untouched()
    bad_radius = (float("nan"), float("inf"), -1.0)
    for fn in (L.vx_field_sphere_trace, L.vx_field_sphere_trace_device):
        assert fn(None, C.byref(trace_args())) == INVALID_ARG
        assert fn(f.h, None) == INVALID_ARG
        assert fn(f.h, C.byref(trace_args(rays_=None))) == INVALID_ARG
        assert fn(f.h, C.byref(trace_args(names=()))) == INVALID_ARG
        for x in (-0.25, 1.0000001, float("nan"), float("inf")):
            assert fn(f.h, C.byref(trace_args(step_scale=x))) == INVALID_ARG, x
        for x in (-1e-9, float("nan"), float("inf")):
            assert fn(f.h, C.byref(trace_args(hit_eps=x))) == INVALID_ARG, x
        assert fn(f.h, C.byref(trace_args(max_steps=65536))) == INVALID_ARG
        for x in bad_radius:
            assert fn(f.h, C.byref(trace_args(radius=x))) == INVALID_ARG, x
        assert fn(f.h, C.byref(trace_args(num=0))) == 0
        assert untouched()
    # a bad global radius beside radius_per_ray is not read
    rpr = np.zeros(n, dtype=F)
    assert L.vx_field_sphere_trace(f.h, C.byref(trace_args(radius=-1.0, radius_per_ray=rpr.ctypes.data))) == 0
    same_bits(outs["status"], fr.sphere_trace(proto["S"], proto["org"], proto["vs"], rays)[3], "status")


def test_default_paths_queue_no_field_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    g.trace(vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1))
    names = list(gpu.profile_read())
    assert names and not any("k_field" in n for n in names), names
    gpu.profile_reset()
    f = g.field()
    f.sample(np.zeros((4, 3), dtype=F))
    f.sphere_trace(np.ones((4, 6), dtype=F))
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert "k_field_sample" in names and "k_field_trace" in names, names


# ---- C++ facade and CLI -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rotcube(gpu, tmp_path_factory):
    """the rotated cube at 0.09 as an OBJ file, its Python field, points (some non-finite, some far outside) and rays"""
    d = tmp_path_factory.mktemp("field_cli")
    v, t = vx_scenes.scene("rotcube")
    obj = d / "r.obj"
    vx_scenes.write_obj(str(obj), v, t)
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.09), gpu.GRID_BOOL)
    S, org, vs, dims = geometry(g)
    pts = np.concatenate([fc.edge_points(dims, org, vs), fc.random_points(dims, org, vs, 1000, 1)])
    return dict(dir=d, obj=str(obj), g=g, f=g.field(), org=org, vs=vs, dims=dims, pts=pts, rays=fc.random_rays(dims, org, vs, 1000, 2))


def test_facade_matches_python(gpu, rotcube):
    import build as vxbuild
    c = rotcube
    exe = str(c["dir"] / "field_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "field_facade.cpp"), "-o", exe, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    pf, rf, out = c["dir"] / "p.f32", c["dir"] / "r.f32", c["dir"] / "o.bin"
    pf.write_bytes(c["pts"].tobytes())
    rf.write_bytes(c["rays"].tobytes())
    radius = float(F(0.05))
    r = subprocess.run([exe, c["obj"], repr(float(F(0.09))), str(pf), str(rf), repr(radius), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    a = c["f"].sample(c["pts"])
    b = c["f"].sphere_trace(c["rays"], radius=radius)
    assert (b["status"] == fr.HIT).any() and (b["status"] == fr.MISS).any()
    part = a["value"].tobytes() + a["gradient"].tobytes() + b["t"].tobytes() + b["status"].tobytes()
    raw = out.read_bytes()
    assert len(raw) == 3 * len(part)
    for k in range(3):
        assert raw[k * len(part):(k + 1) * len(part)] == part, "flavour %d" % k


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


@pytest.mark.parametrize("grid", ["bool", "vec"])
def test_cli_probe(gpu, rotcube, grid):
    c = rotcube
    pin, pout = c["dir"] / "points.txt", c["dir"] / ("probe_%s.txt" % grid)
    pin.write_text("".join("%.9g %.9g %.9g\n" % tuple(p) for p in c["pts"]))
    r = run_cli([c["obj"], "0.09", "--grid", grid, "--probe", str(pin), "--probe-out", str(pout)])
    assert r.returncode == 0, r.stdout
    rows = np.array([[float(x) for x in ln.split()] for ln in pout.read_text().splitlines()])
    assert rows.shape == (len(c["pts"]), 8)
    a = c["f"].sample(c["pts"])
    same_bits(rows[:, :3].astype(F), c["pts"], "points")
    value = rows[:, 3].astype(F)
    nan = np.isnan(a["value"])
    assert nan.any() and np.array_equal(np.isnan(value), nan)  # (the text form of a NaN carries no payload)
    same_bits(value[~nan], a["value"][~nan], "value")
    same_bits(rows[:, 4:7].astype(F), a["gradient"], "gradient")
    assert np.array_equal(rows[:, 7].astype(np.uint8), a["occupied"])
    assert "[voxhip] probe: %d points, %d in occupied cells" % (len(c["pts"]), int(a["occupied"].sum())) in r.stdout


def camera_rays(vi, pi, W, H):
    """the ray of every pixel as the ray kernels generate it, in float32 and in their order"""
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    u = ((px.reshape(-1).astype(F) + F(0.5)) / F(W)).astype(F)
    v = ((py.reshape(-1).astype(F) + F(0.5)) / F(H)).astype(F)
    ndx, ndy = (u * F(2) - F(1)).astype(F), (v * F(2) - F(1)).astype(F)
    tg = [((pi[k] * ndx + pi[4 + k] * ndy).astype(F) + F(pi[8 + k] * F(1) + pi[12 + k] * F(1))).astype(F) for k in range(3)]
    il = (F(1) / np.sqrt(((tg[0] * tg[0] + tg[1] * tg[1]).astype(F) + tg[2] * tg[2]).astype(F))).astype(F)
    n = [(t * il).astype(F) for t in tg]
    d = [((vi[k] * n[0] + vi[4 + k] * n[1]).astype(F) + vi[8 + k] * n[2]).astype(F) for k in range(3)]
    o = [np.full(W * H, vi[12 + k], dtype=F) for k in range(3)]
    return np.stack(o + d, axis=1).astype(F)


def test_cli_sphere_depth(gpu, rotcube):
    c = rotcube
    W, H = 96, 54
    pgm, cam = c["dir"] / "depth.pgm", c["dir"] / "cam.bin"
    radius = F(0.11)
    r = run_cli([c["obj"], "0.09", "--sphere-depth", str(pgm), "--radius", repr(float(radius)), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)])
    assert r.returncode == 0, r.stdout
    m = np.frombuffer(cam.read_bytes(), dtype=F)
    rays = camera_rays(m[:16], m[16:32], W, H)
    b = c["f"].sphere_trace(rays, radius=float(radius))
    hit = b["status"] == fr.HIT
    assert hit.any() and not hit.all()
    q = (b["t"] / c["vs"]).astype(F) * F(16)
    want = np.where(hit, np.where(q < F(65534), q.astype(np.uint32) + 1, 65535), 0).astype(np.uint32)
    raw = pgm.read_bytes()
    head = b"P5\n%d %d\n65535\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + 2 * W * H
    got = np.frombuffer(raw[len(head):], dtype=">u2").astype(np.uint32)
    assert np.array_equal(got, want), int((got != want).sum())
    assert "[voxhip] sphere depth %dx%d: radius" % (W, H) in r.stdout and "%d hits" % int(hit.sum()) in r.stdout


@pytest.mark.parametrize("args", [["--probe", "p.txt", "--grid", "octree"], ["--sphere-depth", "d.pgm"], ["--sphere-depth", "d.pgm", "--radius", "-1"],
                                  ["--radius", "1"], ["--probe-out", "o.txt"], ["--probe", "p.txt", "--bench", "2"]])
def test_cli_refusals(gpu, rotcube, args):
    r = run_cli([rotcube["obj"], "0.09"] + args)
    assert r.returncode == 2 and ("--probe" in r.stdout or "--radius" in r.stdout), r.stdout
