"""GPU tests of the surface mesh (vx_grid_surface*): every output is compared whole, bit for bit, with the restatement (tests/surface_ref.py)
of the GPU's own bitmask, and the mesh is tied to what the library already does (ray tracing, the OBJ loader, the C++ facade)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import surface_ref as sr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY, UNSUPPORTED = 1, 8, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")


def scene(name):
    if name == "torus":
        return vx_scenes.torus()
    if name == "nested":
        return vx_scenes.nested_shells()
    if name == "holed":
        return vx_scenes.holed_box(0.3)
    return vx_scenes.scene(name)


def expected(g, materials=False):
    d = g.describe()
    cells = sr.unpack(g.bitmask(), d["dim"])
    ids = g.materials()[1] if materials else None
    return cells, sr.surface(cells, d["origin"], F(d["voxel_size"]), cell_ids=ids)


def check_surface(g, materials=False, device=True):
    """host and device arrays of the grid against the restatement of its own bitmask"""
    cells, want = expected(g, materials)
    got = g.surface(materials=materials)
    assert len(got) == len(want)
    for a, b, name in zip(got, want, ("verts", "tris", "mats")):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s differ at %d entries" % (name, int((a != b).sum()))
    if device:
        import torch
        dev = g.surface_device(materials=materials)
        torch.cuda.synchronize()
        for a, b in zip(dev, want):
            assert a.cpu().numpy().tobytes() == b.tobytes()
    return cells, want


MESH_CASES = [("blob70k", 2.0 / 64), ("torus", 0.05), ("nested", 0.07), ("holed", 0.09)]


@pytest.mark.parametrize("name,vs", MESH_CASES)
@pytest.mark.parametrize("solid", [False, True])
def test_mesh_surfaces(gpu, name, vs, solid):
    v, t = scene(name)
    mesh = gpu.Mesh.from_arrays(v, t)
    first = None
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, F(vs), kind, solid=solid)
        cells, want = check_surface(g, device=kind == gpu.GRID_BOOL)
        assert cells.any() and len(want[1]) > 0
        if first is None:
            first = want
        assert all(a.tobytes() == b.tobytes() for a, b in zip(want, first))  # the flavours share the bitmask


def test_atrium_512(gpu):
    v, t = vx_scenes.atrium()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(32.0 / 512), gpu.GRID_BOOL)
    assert max(g.describe()["dim"]) >= 500
    check_surface(g)


# ---- masks written from outside -----------------------------------------------------------------------------------------------
def masked_grid(gpu, cells, kind=None, vs=F(0.5)):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, vs, (0.25, -1.0, 3.0))
    write_mask(g, sr.pack(cells))
    g.refresh()
    return g


def test_spiral_maze(gpu):
    cells = vx_scenes.spiral_maze(64)
    g = masked_grid(gpu, cells)
    check_surface(g)
    g.fill_interior()
    check_surface(g)


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 1000), (33, 1, 7), (97, 45, 31), (64, 64, 64), (70000, 2, 2), (3, 40000, 3),
                                  (5, 3, 30000)])
@pytest.mark.parametrize("density", [0.0, 0.01, 0.5, 1.0])
def test_random_masks(gpu, dims, density):
    X, Y, Z = dims
    cells = np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density
    g = masked_grid(gpu, cells, vs=F(0.37))
    got, (v, t) = check_surface(g, device=density == 0.5)
    assert np.array_equal(got, cells)
    if not cells.any():
        assert len(v) == 0 and len(t) == 0
    if cells.all():  # the outer box only
        assert len(t) == 4 * (X * Y + Y * Z + X * Z)


def test_failed_build_is_empty_and_ok(gpu):
    import torch
    v, t = vx_scenes.cube()
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, F(0.25))
    with pytest.raises(gpu.VxError):
        g.revoxelize(mesh, F(2.0 / ((1 << 21) + 4096)))
    assert g.describe()["dim"] == (0, 0, 0)
    L = gpu.lib()
    hv = np.full(12, 7.0, np.float32)
    ht = np.full(12, 5, np.int32)
    nv, nt = ctypes.c_uint64(3), ctypes.c_uint64(4)
    assert L.vx_grid_surface(g.h, hv.ctypes.data, 4, ht.ctypes.data, 4, None, ctypes.byref(nv), ctypes.byref(nt)) == 0
    assert nv.value == 0 and nt.value == 0
    dv = torch.full((12,), 3.0, device="cuda")
    assert L.vx_grid_surface_device(g.h, dv.data_ptr(), 4, dv.data_ptr(), 4, None, ctypes.byref(nv), ctypes.byref(nt)) == 0
    torch.cuda.synchronize()
    assert (hv == 7.0).all() and (ht == 5).all() and (dv.cpu() == 3.0).all()
    vv, tt = g.surface()
    assert vv.shape == (0, 3) and tt.shape == (0, 3)
    assert g.surface_mesh().num_triangles == 0


# ---- the handle's life --------------------------------------------------------------------------------------------------------
def test_rebuilds_set_voxel_fill_and_allocations(gpu):
    v, t = vx_scenes.nested_shells()
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, F(0.07), gpu.GRID_BOOL)
    check_surface(g)
    X, Y, Z = g.describe()["dim"]
    g.set_voxel(X // 2, Y // 2, Z // 2)
    g.set_voxel(0, 0, 0)
    check_surface(g)
    assert g.fill_interior() > 0
    check_surface(g)
    g.revoxelize(mesh, F(0.05), solid=True)
    assert g.describe()["dim"] != (X, Y, Z)
    check_surface(g)
    n0 = gpu.device_allocations()
    for _ in range(3):
        g.surface()
        g.surface_device()
    assert gpu.device_allocations() == n0, "a repeated call at the same dimensions allocated"


def test_non_default_stream(gpu):
    import torch
    v, t = vx_scenes.blob()
    st = torch.cuda.Stream()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 97), gpu.GRID_BOOL, stream=st.cuda_stream)
    hv, ht = g.surface()
    with torch.cuda.stream(st):
        dv, dt = g.surface_device()
    st.synchronize()
    assert dv.cpu().numpy().tobytes() == hv.tobytes() and dt.cpu().numpy().tobytes() == ht.tobytes()
    check_surface(g, device=False)


def _same_desc(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


def material_mesh(gpu, k=3):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    ids = (np.arange(len(t)) % k).astype(np.int32)
    recs = np.zeros(k, gpu.MATERIAL)
    for i in range(k):
        recs[i]["diffuse"] = (0.1 * i, 0.2, 0.3)
        recs[i]["shininess"] = 1.0 + i
    mesh.set_materials(recs, ids)
    return mesh


def test_no_side_effects_on_async_list(gpu):
    mesh = material_mesh(gpu)
    vs = F(2.0 / 64)
    a = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    b = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    a.revoxelize(mesh, vs, materials=True, list_async=True)
    b.revoxelize(mesh, vs, materials=True, list_async=True)
    b.surface()
    b.surface_device()
    assert _same_desc(a.describe(), b.describe()) and np.array_equal(a.bitmask(), b.bitmask())
    assert a.aabbs().tobytes() == b.aabbs().tobytes()
    ma, ia = a.materials()
    mb, ib = b.materials()
    assert ma.tobytes() == mb.tobytes() and ia.tobytes() == ib.tobytes()


@pytest.mark.parametrize("solid", [False, True])
def test_materials(gpu, solid):
    mesh = material_mesh(gpu)
    vs = F(2.0 / 64)
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT):
        g = gpu.Grid.voxelize(mesh, vs, kind, materials=True, solid=solid)
        _, (v, t, m) = check_surface(g, materials=True)
        assert len(np.unique(m)) > 1
        recs, _ = g.materials()
        sm = g.surface_mesh(materials=True)
        mr, mi = sm.materials()
        assert mr.tobytes() == recs.tobytes() and mi.tobytes() == m.tobytes()
        hv, ht = sm.host_arrays()
        assert hv.tobytes() == v.tobytes() and ht.tobytes() == t.tobytes()
    L = gpu.lib()
    probe = np.full(4, -7, np.int32)
    nv, nt = ctypes.c_uint64(), ctypes.c_uint64()
    vec = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    plain_vec = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)
    plain = gpu.Grid.voxelize(mesh, vs, gpu.GRID_BOOL)
    for g, st in ((vec, UNSUPPORTED), (plain_vec, UNSUPPORTED), (plain, INVALID_ARG)):
        assert L.vx_grid_surface(g.h, None, 0, None, 0, probe.ctypes.data, ctypes.byref(nv), ctypes.byref(nt)) == st
        h = ctypes.c_void_p()
        assert L.vx_grid_surface_mesh(g.h, 1, ctypes.byref(h)) == st and h.value is None
        assert (probe == -7).all()
    v0, _ = plain.surface()
    assert len(v0) > 0


def test_capacity_and_argument_errors_write_nothing(gpu):
    import torch
    cells = np.random.default_rng(4).random((5, 6, 7)) < 0.3
    g = masked_grid(gpu, cells)
    want_v, want_t = sr.surface(cells, (0.25, -1.0, 3.0), F(0.5))
    V, T = len(want_v), len(want_t)
    L = gpu.lib()
    nv, nt = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.vx_grid_surface(g.h, None, 0, None, 0, None, ctypes.byref(nv), ctypes.byref(nt)) == 0
    assert (nv.value, nt.value) == (V, T)
    hv = np.full(3 * V, 9.5, np.float32)
    ht = np.full(3 * T, -3, np.int32)
    hm = np.full(T, -4, np.int32)
    for args, st in (((hv.ctypes.data, V - 1, ht.ctypes.data, T), CAPACITY), ((hv.ctypes.data, V, ht.ctypes.data, T - 1), CAPACITY),
                     ((None, V, ht.ctypes.data, T), INVALID_ARG), ((hv.ctypes.data, V, None, T), INVALID_ARG)):
        nv.value = nt.value = 0
        assert L.vx_grid_surface(g.h, args[0], args[1], args[2], args[3], None, ctypes.byref(nv), ctypes.byref(nt)) == st
        if st == CAPACITY:
            assert (nv.value, nt.value) == (V, T)
    assert L.vx_grid_surface(g.h, hv.ctypes.data, V, ht.ctypes.data, T, hm.ctypes.data, ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARG
    assert (hv == 9.5).all() and (ht == -3).all() and (hm == -4).all()
    dv = torch.full((3 * V,), 9.5, device="cuda")
    dt = torch.full((3 * T,), -3, dtype=torch.int32, device="cuda")
    assert L.vx_grid_surface_device(g.h, dv.data_ptr(), V - 1, dt.data_ptr(), T, None, ctypes.byref(nv), ctypes.byref(nt)) == CAPACITY
    assert L.vx_grid_surface_device(g.h, dv.data_ptr(), V, dt.data_ptr(), T - 1, None, ctypes.byref(nv), ctypes.byref(nt)) == CAPACITY
    assert L.vx_grid_surface_device(g.h, None, V, dt.data_ptr(), T, None, ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARG
    assert L.vx_grid_surface_device(None, dv.data_ptr(), V, dt.data_ptr(), T, None, ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARG
    torch.cuda.synchronize()
    assert (dv.cpu() == 9.5).all() and (dt.cpu() == -3).all()
    # exact capacities write exactly the arrays
    assert L.vx_grid_surface(g.h, hv.ctypes.data, V, ht.ctypes.data, T, None, ctypes.byref(nv), ctypes.byref(nt)) == 0
    assert hv.tobytes() == want_v.tobytes() and ht.tobytes() == want_t.tobytes()


# ---- cross-checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vs", [("blob70k", 2.0 / 64), ("torus", 0.05), ("nested", 0.07)])
@pytest.mark.parametrize("solid", [False, True])
def test_tracing_the_mesh_matches_tracing_the_grid(gpu, name, vs, solid):
    v, t = scene(name)
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(vs), gpu.GRID_BOOL, solid=solid)
    d = g.describe()
    X, Y, Z = d["dim"]
    cells = sr.unpack(g.bitmask(), d["dim"])
    occ = np.flatnonzero(cells.reshape(-1))
    _, _, fcell, fd = sr.surface_lattice(cells)
    mesh = g.surface_mesh()
    bvh = gpu.Bvh(mesh)
    org = np.asarray(d["origin"], np.float32)
    bmin, bmax = org - F(0.5), org + np.array([X, Y, Z], np.float32) * F(vs) + F(0.5)
    rays = vx_scenes.random_rays(200000, bmin, bmax, seed=5)
    tg, pg, _ = g.trace(rays)
    tm, pm, _ = bvh.trace(rays)
    hit_g, hit_m = tg > 0, tm > 0
    # a ray through the shared edge of two diagonal cells may touch the boxes and slip between the quads (or the other way round): such
    # rays differ in hit / miss or in t; together they stay within 0.01 % of the rays
    close = np.abs(tg - tm) <= 1e-5 * np.maximum(1.0, tg)
    agree = (hit_g == hit_m) & (~hit_g | close)
    assert agree.mean() >= 0.9999, ((hit_g != hit_m).sum(), (hit_g & hit_m & ~close).sum())
    both = hit_g & hit_m & close
    assert both.sum() > 1000
    # the hit cell, away from the borders of the face hit
    face = pm[both] // 2
    cell_m = fcell[face]
    cell_g = occ[pg[both]]
    r = rays.reshape(-1, 6)[both]
    p = r[:, :3] + tm[both][:, None] * r[:, 3:]
    u = (p - org[None, :]) / F(vs)     # lattice coordinates of the hit point (lattice point i lies at org + i vs)
    axis = fd[face] // 2
    frac = np.abs(u - np.round(u))
    other = np.ones_like(frac, bool)
    other[np.arange(len(axis)), axis] = False
    inner = (frac[other].reshape(-1, 2) > 1e-3).all(axis=1)
    assert inner.mean() > 0.9
    bad = np.flatnonzero(cell_m[inner] != cell_g[inner])
    assert len(bad) == 0, (len(bad), inner.sum(), cell_m[inner][bad[:5]], cell_g[inner][bad[:5]], frac[inner][bad[:5]])


def test_default_paths_queue_no_surface_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    rays = vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1)
    g.trace(rays)
    names = list(gpu.profile_read())
    gpu.profile_reset()
    g.surface()
    surf = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any("surf" in n for n in names), names
    assert any("k_surf_emit" in n for n in surf) and any("k_surf_count" in n for n in surf), surf


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def material_obj(tmp_path):
    v, t = vx_scenes.nested_shells()
    obj = tmp_path / "n.obj"
    (tmp_path / "n.mtl").write_text("newmtl red\nKd 0.8 0.1 0.1\nNs 12\nnewmtl blue\nKd 0.1 0.1 0.9\nKa 0.2 0.2 0.2\nd 0.5\nillum 2\n")
    half = len(t) // 2
    with open(obj, "w") as fh:
        fh.write("mtllib n.mtl\n")
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()))
        fh.write("usemtl red\n")
        fh.write("".join("f %d %d %d\n" % tuple(x + 1 for x in f) for f in t[:half].tolist()))
        fh.write("usemtl blue\n")
        fh.write("".join("f %d %d %d\n" % tuple(x + 1 for x in f) for f in t[half:].tolist()))
    return obj


@pytest.mark.parametrize("grid,materials", [("bool", False), ("aabbstruct", False), ("vec", False), ("bool", True), ("aabbstruct", True)])
def test_cli_obj_round_trip(gpu, tmp_path, grid, materials):
    obj = material_obj(tmp_path)
    out = tmp_path / "s.obj"
    solid = not materials  # (a solid fill hides the inner shell, and with it the second material)
    r = run_cli([str(obj), "0.07", "--grid", grid, "--surface", str(out)] + (["--solid"] if solid else []) + (["--materials"] if materials else []))
    assert r.returncode == 0, r.stdout
    kind = {"bool": gpu.GRID_BOOL, "aabbstruct": gpu.GRID_AABBSTRUCT, "vec": gpu.GRID_VEC}[grid]
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.07), kind, solid=solid, materials=materials)
    want = g.surface(materials=materials)
    back = gpu.Mesh.load_obj(str(out))
    hv, ht = back.host_arrays()
    assert hv.tobytes() == want[0].tobytes() and ht.tobytes() == want[1].tobytes()
    if materials:
        recs, _ = g.materials()
        mr, mi = back.materials()
        assert mi.tobytes() == want[2].tobytes()
        for f in ("ambient", "diffuse", "specular", "transmittance", "emission", "shininess", "ior", "dissolve", "illum"):
            assert mr[f].tobytes() == recs[f].tobytes(), f
        assert len(np.unique(want[2])) > 1
    else:
        assert not (tmp_path / "s.mtl").exists()


def build_facade_program(tmp_path):
    import build as vxbuild
    src = tmp_path / "surface_facade.cpp"
    src.write_text(r'''
#include <cstdio>
#include <fstream>
#include <string>
#include "VoxelBuilder.hpp"
int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    VoxelBuilder<VoxelGridBool> vb{std::filesystem::path(argv[1])};
    vb.withMaterials(true);
    const VoxelGridBool g = vb.buildVoxelGrid(std::stof(argv[2]));
    std::vector<float> xyz;
    std::vector<int32_t> tris, mats;
    g.surface(xyz, tris, &mats);
    std::ofstream f(argv[3], std::ios::binary);
    f.write(reinterpret_cast<const char*>(xyz.data()), (std::streamsize)(xyz.size() * 4));
    f.write(reinterpret_cast<const char*>(tris.data()), (std::streamsize)(tris.size() * 4));
    f.write(reinterpret_cast<const char*>(mats.data()), (std::streamsize)(mats.size() * 4));
    std::printf("%zu %zu\n", xyz.size() / 3, tris.size() / 3);
    return f ? 0 : 1;
}
''')
    out = str(tmp_path / "surface_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           str(src), "-o", out, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    return out


def test_facade_matches_python(gpu, tmp_path):
    exe = build_facade_program(tmp_path)
    obj = material_obj(tmp_path)
    out = tmp_path / "f.bin"
    r = subprocess.run([exe, str(obj), "0.07", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.07), gpu.GRID_BOOL, materials=True)
    v, t, m = g.surface(materials=True)
    assert out.read_bytes() == v.tobytes() + t.tobytes() + m.tobytes()
