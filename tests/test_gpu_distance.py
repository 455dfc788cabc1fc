"""GPU tests of the distance fields (vx_grid_distance_sq*, vx_grid_sdf*): every field is compared whole, bit for bit, with the restatement
(tests/distance_ref.py) of the GPU's own bitmask."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")


def scene(name):
    if name == "torus":
        return vx_scenes.torus()
    if name == "nested":
        return vx_scenes.nested_shells()
    return vx_scenes.scene(name)


def check_fields(g, fast=True, device=True):
    """D_out, D_in and s of the grid against the restatement of its own bitmask; host and device variants bit-equal."""
    d = g.describe()
    dim, vs = d["dim"], d["voxel_size"]
    w = g.bitmask()
    m = dr.unpack(w, dim)
    f = dr.edt_sq_c if fast else dr.edt_sq
    d_out, d_in = f(m), f(~m)
    assert np.array_equal(g.distance_sq(), d_out), "D_out: %d cells differ" % int((g.distance_sq() != d_out).sum())
    assert np.array_equal(g.distance_sq(inside=True), d_in), "D_in differs"
    s = dr.sdf_from(m, d_out, d_in, vs)
    got = g.sdf()
    assert got.tobytes() == s.tobytes(), "sdf: %d cells differ" % int((got.view(np.uint32) != s.view(np.uint32)).sum())
    if device:
        import torch
        a = g.distance_sq_device()
        b = g.distance_sq_device(inside=True)
        c = g.sdf_device()
        torch.cuda.synchronize()
        assert a.dtype == torch.uint32 and tuple(a.shape) == m.shape and c.dtype == torch.float32
        assert np.array_equal(a.view(torch.int32).cpu().numpy().view(np.uint32), d_out)
        assert np.array_equal(b.view(torch.int32).cpu().numpy().view(np.uint32), d_in)
        assert c.cpu().numpy().tobytes() == s.tobytes()
    return m, d_out, d_in, s


MESH_CASES = [("cube", 0.25), ("rotcube", 0.09), ("blob70k", 2.0 / 64), ("blob70k", 2.0 / 97), ("torus", 0.05), ("nested", 0.07)]


@pytest.mark.parametrize("name,vs", MESH_CASES)
@pytest.mark.parametrize("solid", [False, True])
def test_mesh_fields(gpu, name, vs, solid):
    v, t = scene(name)
    mesh = gpu.Mesh.from_arrays(v, t)
    first = None
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, F(vs), kind, solid=solid)
        m, d_out, d_in, s = check_fields(g, device=kind == gpu.GRID_BOOL)
        if first is None:
            first = s
            assert m.any() and (not solid or name in ("cube",) or (d_in > 1).any())
        assert s.tobytes() == first.tobytes()  # the flavours share the bitmask


def test_atrium_512(gpu):
    v, t = vx_scenes.atrium()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(32.0 / 512), gpu.GRID_BOOL, solid=True)
    assert max(g.describe()["dim"]) >= 500
    check_fields(g, fast=True, device=False)


# ---- masks written from outside -----------------------------------------------------------------------------------------------
def masked_grid(gpu, cells, kind=None, vs=F(0.5)):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, vs, (0.25, -1.0, 3.0))
    write_mask(g, dr.pack(cells))
    g.refresh()
    return g


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 1000), (33, 1, 7), (97, 45, 31), (64, 64, 64)])
@pytest.mark.parametrize("density", [0.0, 1e-4, 0.01, 0.5, 1.0])
def test_random_masks(gpu, dims, density):
    X, Y, Z = dims
    cells = np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density
    g = masked_grid(gpu, cells, vs=F(0.37))
    m, d_out, d_in, s = check_fields(g, fast=False)
    assert np.array_equal(m, cells)
    if not cells.any():
        assert (d_out == 0xFFFFFFFF).all() and (s == np.inf).all()
    if cells.all():
        assert (d_in == 0xFFFFFFFF).all() and (s == -np.inf).all()


def test_long_x_axis_at_the_limit(gpu):
    g = gpu.Grid.create(gpu.GRID_BOOL, 65536, 2, 2, F(0.01))
    for c in ((0, 0, 0), (65535, 1, 1), (32768, 0, 1)):
        g.set_voxel(*c)
    _, d_out, d_in, s = check_fields(g)
    assert d_out[0, 0, 16384] == 16384 ** 2 and d_out[1, 1, 0] == 2 and d_out[0, 1, 65535] == 1 and d_out.max() == 16384 ** 2 + 1
    assert s[0, 0, 0] == -F(0.01) and (d_in[d_out == 0] == 1).all()


@pytest.mark.parametrize("dims", [(3, 40000, 3), (5, 3, 60000)])
def test_long_columns(gpu, dims):
    X, Y, Z = dims
    rng = np.random.default_rng(11)
    cells = rng.random((Z, Y, X)) < 2e-4
    cells[0, 0, 0] = True
    g = masked_grid(gpu, cells)
    check_fields(g)
    cells = ~cells  # and mostly occupied: D_in carries the long runs
    g = masked_grid(gpu, cells)
    check_fields(g)


@pytest.mark.parametrize("dims", [(2, 1024, 520), (1024, 2, 520), (1024, 520, 2)])
def test_grid_stride_loops(gpu, dims):
    """more rows, more y columns and more z columns than the 2048 x 256 threads of a launch: the signed kernels' loops go round too"""
    X, Y, Z = dims
    assert max(Y * Z, X * Z, X * Y) > 2048 * 256
    cells = np.random.default_rng(X + 2 * Y).random((Z, Y, X)) < 0.01
    g = masked_grid(gpu, cells)
    check_fields(g, device=False)


def misaligned_out(n, dtype, canary):
    """a contiguous device tensor of n elements that starts 4 bytes past a 16-byte boundary, between two canaries -> (whole, slice)"""
    import torch
    big = torch.full((n + 2,), canary, dtype=dtype, device="cuda")
    out = big[1:1 + n]
    assert big.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    return big, out


def test_misaligned_device_output(gpu):
    """X % 4 == 0, but the output is only 4-byte aligned: the x pass takes its scalar stores because of the pointer.  Every field equals
    its host variant (whose staging buffer is aligned) bit for bit, and nothing is written outside the n elements."""
    import torch
    cells = np.random.default_rng(64).random((3, 5, 64)) < 0.3
    g = masked_grid(gpu, cells)
    n = cells.size
    for inside in (False, True):
        big, out = misaligned_out(n, torch.int32, 0x5A5A5A5A)
        g.distance_sq_device(out=out.view(3, 5, 64), inside=inside)
        torch.cuda.synchronize()
        got = big.cpu().numpy()
        assert got[0] == 0x5A5A5A5A and got[n + 1] == 0x5A5A5A5A
        assert np.array_equal(got[1:1 + n].view(np.uint32), g.distance_sq(inside=inside).reshape(-1)), inside
    big, out = misaligned_out(n, torch.float32, 7.5)
    g.sdf_device(out=out)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert got[0] == 7.5 and got[n + 1] == 7.5
    assert got[1:1 + n].tobytes() == g.sdf().tobytes()


def test_over_the_limit_is_refused(gpu):
    import torch
    g = gpu.Grid.create(gpu.GRID_BOOL, 65537, 1, 1, F(0.01))
    g.set_voxel(3, 0, 0)
    L = gpu.lib()
    host = np.full(65537, 0xABCDEF01, np.uint32)
    assert L.vx_grid_distance_sq(g.h, 0, host.ctypes.data, host.size) == CAPACITY
    hf = np.full(65537, 7.0, np.float32)
    assert L.vx_grid_sdf(g.h, hf.ctypes.data, hf.size) == CAPACITY
    dev = torch.full((65537,), -5, dtype=torch.int32, device="cuda")
    assert L.vx_grid_distance_sq_device(g.h, 0, dev.data_ptr(), dev.numel()) == CAPACITY
    assert L.vx_grid_sdf_device(g.h, dev.data_ptr(), dev.numel()) == CAPACITY
    torch.cuda.synchronize()
    assert (host == 0xABCDEF01).all() and (hf == 7.0).all() and (dev.cpu() == -5).all()
    with pytest.raises(gpu.VxError):
        g.sdf()


# ---- the handle's life --------------------------------------------------------------------------------------------------------
def test_rebuilds_and_allocations(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, F(2.0 / 97), gpu.GRID_BOOL)
    check_fields(g)
    g.revoxelize(mesh, F(2.0 / 64), solid=True)
    check_fields(g)
    n0 = gpu.device_allocations()
    for _ in range(3):
        g.distance_sq()
        g.distance_sq(inside=True)
        g.sdf()
        g.distance_sq_device()
    assert gpu.device_allocations() == n0, "a repeated call at the same dimensions allocated"
    # a flat, non-cubic grid from a mask after that
    cells = np.random.default_rng(2).random((7, 40, 130)) < 0.05
    h = masked_grid(gpu, cells)
    check_fields(h)
    g2 = masked_grid(gpu, cells)
    g2.sdf()
    write_mask(g2, dr.pack(np.zeros_like(cells)))
    g2.refresh()
    check_fields(g2)


def test_after_set_voxel_and_fill_interior(gpu):
    v, t = vx_scenes.nested_shells()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(0.07), gpu.GRID_BOOL)
    check_fields(g)
    X, Y, Z = g.describe()["dim"]
    g.set_voxel(X // 2, Y // 2, Z // 2)
    g.set_voxel(0, 0, 0)
    check_fields(g)
    assert g.fill_interior() > 0
    check_fields(g)


def test_failed_build_is_empty_and_ok(gpu):
    import torch
    v, t = vx_scenes.cube()
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, F(0.25))
    with pytest.raises(gpu.VxError):
        g.revoxelize(mesh, F(2.0 / ((1 << 21) + 4096)))
    assert g.describe()["dim"] == (0, 0, 0)
    L = gpu.lib()
    host = np.full(4, 9, np.uint32)
    assert L.vx_grid_distance_sq(g.h, 0, host.ctypes.data, 0) == 0
    assert L.vx_grid_sdf(g.h, host.ctypes.data, 0) == 0
    dev = torch.full((4,), 3, dtype=torch.int32, device="cuda")
    assert L.vx_grid_distance_sq_device(g.h, 1, dev.data_ptr(), 0) == 0
    assert L.vx_grid_sdf_device(g.h, dev.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert (host == 9).all() and (dev.cpu() == 3).all()
    assert g.sdf().shape == (0, 0, 0)


def test_no_side_effects_on_async_list_and_materials(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    ids = (np.arange(len(t)) % 3).astype(np.int32)
    recs = np.zeros(3, gpu.MATERIAL)
    for k in range(3):
        recs[k]["diffuse"] = (0.1 * k, 0.2, 0.3)
    mesh.set_materials(recs, ids)
    vs = F(2.0 / 64)
    a = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    b = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    a.revoxelize(mesh, vs, materials=True, list_async=True)
    b.revoxelize(mesh, vs, materials=True, list_async=True)
    b.sdf()
    b.distance_sq_device()
    b.distance_sq(inside=True)
    assert _same_desc(a.describe(), b.describe()) and np.array_equal(a.bitmask(), b.bitmask())
    assert a.aabbs().tobytes() == b.aabbs().tobytes()
    ma, ia = a.materials()
    mb, ib = b.materials()
    assert ma.tobytes() == mb.tobytes() and ia.tobytes() == ib.tobytes()
    # a materials build (not async) too
    c = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    e = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    e.sdf()
    assert c.aabbs().tobytes() == e.aabbs().tobytes()
    assert c.materials()[1].tobytes() == e.materials()[1].tobytes()


def _same_desc(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


def test_non_default_stream(gpu):
    import torch
    v, t = vx_scenes.blob()
    st = torch.cuda.Stream()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 97), gpu.GRID_BOOL, stream=st.cuda_stream)
    s_host = g.sdf()
    with torch.cuda.stream(st):
        out = g.sdf_device()
        out32 = torch.empty(out.shape, dtype=torch.int32, device="cuda")
        g.distance_sq_device(out=out32, inside=True)
    st.synchronize()
    assert out.cpu().numpy().tobytes() == s_host.tobytes()
    assert np.array_equal(out32.cpu().numpy().view(np.uint32), g.distance_sq(inside=True))
    check_fields(g)


def test_argument_errors_write_nothing(gpu):
    import torch
    cells = np.random.default_rng(4).random((5, 6, 7)) < 0.2
    g = masked_grid(gpu, cells)
    L = gpu.lib()
    n = 7 * 6 * 5
    host = np.full(n, 0x12345678, np.uint32)
    assert L.vx_grid_distance_sq(g.h, 0, host.ctypes.data, n - 1) == CAPACITY
    assert L.vx_grid_distance_sq(g.h, 2, host.ctypes.data, n) == INVALID_ARG
    assert L.vx_grid_distance_sq(g.h, 0x80000001, host.ctypes.data, n) == INVALID_ARG
    assert L.vx_grid_distance_sq(g.h, 0, None, n) == INVALID_ARG
    assert L.vx_grid_sdf(g.h, host.ctypes.data, n - 1) == CAPACITY
    assert L.vx_grid_sdf(g.h, None, n) == INVALID_ARG
    assert L.vx_grid_sdf(None, host.ctypes.data, n) == INVALID_ARG
    assert (host == 0x12345678).all()
    dev = torch.full((n,), 0x1234567, dtype=torch.int32, device="cuda")
    assert L.vx_grid_distance_sq_device(g.h, 0, dev.data_ptr(), n - 1) == CAPACITY
    assert L.vx_grid_distance_sq_device(g.h, 4, dev.data_ptr(), n) == INVALID_ARG
    assert L.vx_grid_distance_sq_device(g.h, 0, None, n) == INVALID_ARG
    assert L.vx_grid_distance_sq_device(None, 0, dev.data_ptr(), n) == INVALID_ARG
    assert L.vx_grid_sdf_device(g.h, dev.data_ptr(), n - 1) == CAPACITY
    assert L.vx_grid_sdf_device(g.h, None, n) == INVALID_ARG
    torch.cuda.synchronize()
    assert (dev.cpu() == 0x1234567).all()
    with pytest.raises(ValueError):
        g.sdf_device(out=torch.empty(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        g.distance_sq_device(out=torch.empty(n - 1, dtype=torch.int32, device="cuda"))


# ---- C++ facade and CLI -------------------------------------------------------------------------------------------------------
def build_facade_program(tmp_path):
    import build as vxbuild
    out = str(tmp_path / "distance_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "distance_facade.cpp"), "-o", out, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    return out


@pytest.mark.parametrize("solid", [False, True])
def test_facade_matches_python(gpu, tmp_path, solid):
    exe = build_facade_program(tmp_path)
    v, t = vx_scenes.torus()
    obj = tmp_path / "t.obj"
    vx_scenes.write_obj(str(obj), v, t)
    vs = F(0.05)
    out = tmp_path / "f.bin"
    r = subprocess.run([exe, str(obj), repr(float(vs)), str(out)] + (["solid"] if solid else []), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), vs, gpu.GRID_BOOL, solid=solid)
    s, d = g.sdf(), g.distance_sq(inside=True)
    n = s.size
    raw = out.read_bytes()
    assert len(raw) == 3 * 8 * n
    for k in range(3):
        part = raw[k * 8 * n:(k + 1) * 8 * n]
        assert part[:4 * n] == s.tobytes() and part[4 * n:] == d.tobytes(), "flavour %d" % k


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


@pytest.mark.parametrize("grid", ["bool", "aabbstruct", "vec"])
@pytest.mark.parametrize("solid", [False, True])
def test_cli_sdf(gpu, tmp_path, grid, solid):
    v, t = vx_scenes.nested_shells()
    obj = tmp_path / "n.obj"
    vx_scenes.write_obj(str(obj), v, t)
    f = tmp_path / "s.f32"
    r = run_cli([str(obj), "0.07", "--grid", grid, "--sdf", str(f)] + (["--solid"] if solid else []))
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.07), gpu.GRID_BOOL, solid=solid)
    s = g.sdf()
    X, Y, Z = g.describe()["dim"]
    data = f.read_bytes()
    assert len(data) == 4 * X * Y * Z and data == s.astype("<f4").tobytes()
    fin = s[np.isfinite(s)]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("[voxhip] sdf:")]
    assert len(line) == 1, r.stdout
    mm = re.match(r"\[voxhip\] sdf: (\d+) x (\d+) x (\d+) cells, min (\S+) max (\S+)$", line[0])
    assert mm and tuple(int(x) for x in mm.groups()[:3]) == (X, Y, Z)
    assert np.isclose(float(mm.group(4)), fin.min(), rtol=1e-5) and np.isclose(float(mm.group(5)), fin.max(), rtol=1e-5)


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--bench", "2"]])
def test_cli_sdf_refusals(gpu, tmp_path, extra):
    v, t = vx_scenes.cube()
    obj = tmp_path / "c.obj"
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--sdf", str(tmp_path / "s.f32")] + extra)
    assert r.returncode != 0 and "--sdf" in r.stdout


def test_default_paths_queue_no_distance_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    gi_rays = vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1)
    g.trace(gi_rays)
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any("dist" in n for n in names), names
