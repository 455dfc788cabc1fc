"""GPU tests of connected-component labelling (vx_grid_components*, vx_grid_component_stats): labels, K and statistics are compared whole,
bit for bit, with the restatement (tests/components_ref.py) of the GPU's own bitmask, for 6- and 26-connectivity."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
CONN = (6, 26)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")


def check(g, connectivity=CONN, device=True, cells=None):
    """labels, K and stats of every connectivity against the restatement of the grid's own bitmask; host and device variants bit-equal."""
    dim = g.describe()["dim"]
    m = cr.unpack(g.bitmask(), dim)
    if cells is not None:
        assert np.array_equal(m, cells)
    out = {}
    for c in connectivity:
        want, k = cr.label_c(m, c) if m.size > 1 << 18 else cr.label(m, c)
        got, kg = g.components(c)
        assert kg == k, "connectivity %d: K %d, want %d" % (c, kg, k)
        assert got.shape == m.shape and np.array_equal(got, want), "connectivity %d: %d labels differ" % (c, int((got != want).sum()))
        s = g.component_stats(c)
        assert s.dtype.itemsize == 32 and s.tobytes() == cr.stats(want, k).tobytes(), "connectivity %d: stats differ" % c
        if device:
            import torch
            lab, kd = g.components_device(connectivity=c)
            torch.cuda.synchronize()
            assert lab.dtype == torch.uint32 and tuple(lab.shape) == m.shape
            assert int(kd.item()) == k
            assert np.array_equal(lab.view(torch.int32).cpu().numpy().view(np.uint32), want)
        out[c] = (want, k)
    return m, out


def masked_grid(gpu, cells, kind=None, vs=F(0.5)):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, vs, (0.25, -1.0, 3.0))
    write_mask(g, cr.pack(cells))
    g.refresh()
    return g


def scene(name):
    if name == "torus":
        return vx_scenes.torus()
    if name == "nested":
        return vx_scenes.nested_shells()
    if name == "holed":
        return vx_scenes.holed_box(0.4)
    if name == "soup":
        return vx_scenes.soup(6000, extent=1.0)
    return vx_scenes.scene(name)


MESH_CASES = [("blob70k", 2.0 / 64), ("blob70k", 2.0 / 97), ("torus", 0.05), ("nested", 0.07), ("holed", 0.06), ("soup", 2.0 / 128),
              ("soup", 2.0 / 200)]


@pytest.mark.parametrize("name,vs", MESH_CASES)
@pytest.mark.parametrize("solid", [False, True])
def test_mesh_scenes(gpu, name, vs, solid):
    v, t = scene(name)
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(vs), gpu.GRID_BOOL, solid=solid)
    m, out = check(g)
    assert m.any()
    if name == "soup" and not solid:
        assert out[6][1] > 1000  # thousands of tiny components


def test_flavours_share_labels(gpu):
    v, t = vx_scenes.nested_shells()
    mesh = gpu.Mesh.from_arrays(v, t)
    first = None
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, F(0.07), kind)
        _, out = check(g, device=kind == gpu.GRID_BOOL)
        if first is None:
            first = out
        assert all(np.array_equal(out[c][0], first[c][0]) for c in CONN)


@pytest.mark.parametrize("n,closed", [(96, True), (97, False)])
def test_spiral_maze(gpu, n, closed):
    cells = vx_scenes.spiral_maze(n, closed_core=closed)
    g = masked_grid(gpu, cells)
    _, out = check(g, cells=cells)
    assert out[6][1] > 10  # the nested shells are separate under both connectivities
    h = masked_grid(gpu, ~cells)  # the empty cells: one winding component under 6-connectivity (with the closed core's inside apart)
    _, out = check(h)
    assert out[6][1] == (2 if closed else 1)


def test_atrium_512(gpu):
    v, t = vx_scenes.atrium()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(32.0 / 512), gpu.GRID_BOOL, solid=True)
    assert max(g.describe()["dim"]) >= 500
    check(g)


@pytest.mark.parametrize("dims", [(97, 61, 45), (64, 64, 64), (128, 33, 70), (256, 256, 256)])
@pytest.mark.parametrize("density", [0.10, 0.31, 0.6])
def test_random_masks(gpu, dims, density):
    X, Y, Z = dims
    cells = np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 100)).random((Z, Y, X)) < density
    g = masked_grid(gpu, cells)
    check(g, cells=cells, device=X * Y * Z < 1 << 20)


def test_full_grid(gpu):
    cells = np.ones((130, 150, 200), bool)
    g = masked_grid(gpu, cells)
    _, out = check(g, cells=cells)
    assert out[6][1] == out[26][1] == 1


def test_checkerboard_128(gpu):
    z, y, x = np.indices((128, 128, 128))
    cells = (x + y + z) % 2 == 0
    g = masked_grid(gpu, cells)
    _, out = check(g, cells=cells)
    assert out[6][1] == 1048576 and out[26][1] == 1
    s = g.component_stats(6)
    assert (s["cells"] == 1).all() and (s["min"] == s["max"]).all()


def test_long_x_row(gpu):
    X = 1 << 21
    cells = np.zeros((2, 2, X), bool)
    cells[1, 0, :] = True
    cells[0, 1, 5] = cells[0, 1, X - 1] = True  # two diagonal neighbours of the row (26: one component), apart under 6
    g = masked_grid(gpu, cells)
    _, out = check(g, cells=cells)
    assert out[6][1] == 3 and out[26][1] == 1


def test_long_z_column(gpu):
    Z = 400000
    cells = np.zeros((Z, 3, 3), bool)
    cells[:, 1, 1] = True
    cells[7, 0, 0] = True
    g = masked_grid(gpu, cells)
    _, out = check(g, cells=cells)
    assert out[6][1] == 2 and out[26][1] == 1


# ---- the handle's life --------------------------------------------------------------------------------------------------------
def test_empty_and_failed_build(gpu):
    import torch
    g = masked_grid(gpu, np.zeros((5, 6, 7), bool))
    _, out = check(g)
    assert out[6][1] == 0 and len(g.component_stats(26)) == 0
    v, t = vx_scenes.cube()
    mesh = gpu.Mesh.from_arrays(v, t)
    h = gpu.Grid.voxelize(mesh, F(0.25))
    with pytest.raises(gpu.VxError):
        h.revoxelize(mesh, F(2.0 / ((1 << 21) + 4096)))
    assert h.describe()["dim"] == (0, 0, 0)
    L = gpu.lib()
    k = ctypes.c_uint64(77)
    host = np.full(4, 9, np.uint32)
    assert L.vx_grid_components(h.h, 6, host.ctypes.data, 4, ctypes.byref(k)) == 0 and k.value == 0
    dev = torch.full((4,), 3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.vx_grid_components_device(h.h, 26, dev.data_ptr(), 0, dev.data_ptr()) == 0
    k.value = 5
    assert L.vx_grid_component_stats(h.h, 6, None, 0, ctypes.byref(k)) == 0 and k.value == 0
    torch.cuda.synchronize()
    assert (host == 9).all() and (dev.cpu() == 3).all()
    lab, kk = h.components()
    assert lab.shape == (0, 0, 0) and kk == 0


def test_set_voxel_fill_interior_and_refresh(gpu):
    v, t = vx_scenes.nested_shells()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(0.07), gpu.GRID_BOOL)
    _, out0 = check(g)
    X, Y, Z = g.describe()["dim"]
    g.set_voxel(X // 2, Y // 2, Z // 2)
    g.set_voxel(0, 0, 0)
    _, out1 = check(g)
    assert out1[6][1] >= out0[6][1] + 1
    assert g.fill_interior() > 0
    _, out2 = check(g)
    assert out2[6][1] < out1[6][1]  # the solid: shells, gap and the inner cell are one
    cells = cr.unpack(g.bitmask(), (X, Y, Z)).copy()
    cells[:, :, X // 2] = False  # an external write splits the solid
    write_mask(g, cr.pack(cells))
    g.refresh()
    _, out3 = check(g, cells=cells)
    assert out3[6][1] >= 2


def test_over_the_limit_is_refused(gpu):
    import torch
    L = gpu.lib()
    k = ctypes.c_uint64(123)
    host = np.full(16, 0xABCDEF01, np.uint32)
    dev = torch.full((16,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = np.zeros(2, gpu.COMPONENT)
    st["cells"] = 77
    for dims in ((2048, 2048, 1024), (65536, 65536, 1)):
        g = gpu.Grid.create(gpu.GRID_BOOL, *dims, F(0.01))
        g.set_voxel(3, 0, 0)
        assert L.vx_grid_components(g.h, 6, host.ctypes.data, host.size, ctypes.byref(k)) == CAPACITY
        assert L.vx_grid_components(g.h, 26, None, 0, ctypes.byref(k)) == CAPACITY
        assert L.vx_grid_components_device(g.h, 6, dev.data_ptr(), 1 << 40, dev.data_ptr()) == CAPACITY
        assert L.vx_grid_component_stats(g.h, 6, st.ctypes.data, 2, ctypes.byref(k)) == CAPACITY
        assert L.vx_grid_components(g.h, 7, host.ctypes.data, host.size, ctypes.byref(k)) == INVALID_ARG  # (the argument check comes first)
        del g
    torch.cuda.synchronize()
    assert (host == 0xABCDEF01).all() and (dev.cpu() == -5).all() and (st["cells"] == 77).all() and k.value == 123


def test_1024_cubed_is_accepted(gpu):
    g = gpu.Grid.create(gpu.GRID_BOOL, 1024, 1024, 1024, F(0.01))
    g.set_voxel(1023, 1023, 1023)
    g.set_voxel(5, 6, 7)
    L = gpu.lib()
    k = ctypes.c_uint64()
    assert L.vx_grid_components(g.h, 26, None, 0, ctypes.byref(k)) == 0 and k.value == 2
    s = g.component_stats(6)
    assert s["cells"].tolist() == [1, 1] and tuple(s[0]["min"]) == (5, 6, 7) and tuple(s[1]["max"]) == (1023, 1023, 1023)


def test_argument_errors_write_nothing(gpu):
    import torch
    cells = np.random.default_rng(4).random((5, 6, 7)) < 0.3
    g = masked_grid(gpu, cells)
    _, out = check(g)
    L = gpu.lib()
    n = 7 * 6 * 5
    k6 = out[6][1]
    host = np.full(n, 0x12345678, np.uint32)
    k = ctypes.c_uint64(99)
    for bad in (0, 1, 18, 27, 0x80000006):
        assert L.vx_grid_components(g.h, bad, host.ctypes.data, n, ctypes.byref(k)) == INVALID_ARG
        assert L.vx_grid_component_stats(g.h, bad, None, 0, ctypes.byref(k)) == INVALID_ARG
    assert k.value == 99
    assert L.vx_grid_components(None, 6, host.ctypes.data, n, ctypes.byref(k)) == INVALID_ARG
    assert L.vx_grid_components(g.h, 6, None, n, ctypes.byref(k)) == INVALID_ARG
    assert L.vx_grid_components(g.h, 6, host.ctypes.data, n - 1, ctypes.byref(k)) == CAPACITY and k.value == k6  # count still reported
    k.value = 99
    assert L.vx_grid_components(g.h, 26, host.ctypes.data, 0, ctypes.byref(k)) == CAPACITY and k.value == out[26][1]
    assert (host == 0x12345678).all()
    st = np.zeros(k6, gpu.COMPONENT)
    st["cells"] = 55
    k.value = 99
    assert L.vx_grid_component_stats(g.h, 6, st.ctypes.data, k6 - 1, ctypes.byref(k)) == CAPACITY and k.value == k6
    assert L.vx_grid_component_stats(g.h, 6, None, 3, ctypes.byref(k)) == INVALID_ARG
    assert L.vx_grid_component_stats(None, 6, st.ctypes.data, k6, ctypes.byref(k)) == INVALID_ARG
    assert (st["cells"] == 55).all()
    dev = torch.full((n + 1,), 0x1234567, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.vx_grid_components_device(g.h, 6, dev.data_ptr(), n - 1, dev[n:].data_ptr()) == CAPACITY
    assert L.vx_grid_components_device(g.h, 4, dev.data_ptr(), n, None) == INVALID_ARG
    assert L.vx_grid_components_device(g.h, 6, None, n, None) == INVALID_ARG
    assert L.vx_grid_components_device(None, 6, dev.data_ptr(), n, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert (dev.cpu() == 0x1234567).all()
    # a device call without a count, into an int32 tensor
    assert L.vx_grid_components_device(g.h, 26, dev.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dev[:n].cpu().numpy().view(np.uint32).reshape(cells.shape), out[26][0]) and int(dev[n].item()) == 0x1234567
    with pytest.raises(ValueError):
        g.components_device(out=torch.empty(n - 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(gpu.VxError):
        g.components(18)


def _same_desc(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


def test_no_side_effects(gpu):
    import torch
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    ids = (np.arange(len(t)) % 3).astype(np.int32)
    recs = np.zeros(3, gpu.MATERIAL)
    for j in range(3):
        recs[j]["diffuse"] = (0.1 * j, 0.2, 0.3)
    mesh.set_materials(recs, ids)
    vs = F(2.0 / 64)
    a = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    b = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    a.revoxelize(mesh, vs, materials=True, list_async=True)
    b.revoxelize(mesh, vs, materials=True, list_async=True)
    w0 = b.bitmask()
    b.components(6)
    b.components_device(connectivity=26)
    b.component_stats(26)
    assert _same_desc(a.describe(), b.describe()) and np.array_equal(a.bitmask(), b.bitmask()) and np.array_equal(w0, b.bitmask())
    assert a.aabbs().tobytes() == b.aabbs().tobytes()
    ma, ia = a.materials()
    mb, ib = b.materials()
    assert ma.tobytes() == mb.tobytes() and ia.tobytes() == ib.tobytes()
    # a bound list buffer is untouched by the calls
    c = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)
    n = c.describe()["set_calls"] * 2 + 64
    buf = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.bind_aabbs_device(buf.data_ptr(), n)
    c.revoxelize(mesh, vs)
    torch.cuda.synchronize()
    before = buf.clone()
    c.components(26)
    c.components_device()
    c.component_stats(6)
    torch.cuda.synchronize()
    assert torch.equal(before, buf)
    c.bind_aabbs_device(None, 0)


def test_non_default_stream(gpu):
    import torch
    v, t = vx_scenes.torus()
    st = torch.cuda.Stream()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(0.05), gpu.GRID_BOOL, stream=st.cuda_stream)
    want, k = g.components(26)
    with torch.cuda.stream(st):
        out32 = torch.empty(want.shape, dtype=torch.int32, device="cuda")
        lab, kd = g.components_device(out=out32, connectivity=26)
    st.synchronize()
    assert lab is out32 and int(kd.item()) == k
    assert np.array_equal(out32.cpu().numpy().view(np.uint32), want)
    check(g)


def test_repeated_calls_allocate_nothing_and_agree(gpu):
    import torch
    cells = np.random.default_rng(12).random((256, 256, 256)) < 0.31
    g = masked_grid(gpu, cells)
    for c in CONN:
        g.components(c)
        g.component_stats(c)
        g.components_device(connectivity=c)
    torch.cuda.synchronize()
    n0 = gpu.device_allocations()
    outs = []
    for _ in range(3):
        g.components(6)
        g.component_stats(26)
        lab, _ = g.components_device(connectivity=6)
        torch.cuda.synchronize()
        outs.append(lab.view(torch.int32).cpu().numpy().tobytes())
    assert outs[0] == outs[1] == outs[2]
    del lab
    torch.cuda.synchronize()
    # (the device results come from torch's allocator, so only the library's pool is counted)
    assert gpu.device_allocations() == n0, "a repeated call at the same dimensions allocated"
    want, _ = cr.label_c(cells, 6)
    assert outs[0] == want.view(np.int32).tobytes()


def test_default_paths_queue_no_components_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    rays = vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1)
    g.trace(rays)
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any(n.startswith("k_cc_") for n in names), names


def test_profiler_sees_the_kernels(gpu):
    g = masked_grid(gpu, np.random.default_rng(1).random((20, 30, 40)) < 0.3)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g.component_stats(26)
    names = set(gpu.profile_read())
    gpu.profile_enable(False)
    assert {"k_cc_local", "k_cc_merge", "k_cc_flatten", "k_cc_label", "k_cc_stats"} <= names, names


# ---- C++ facade and CLI -------------------------------------------------------------------------------------------------------
def build_facade_program(tmp_path):
    import build as vxbuild
    out = str(tmp_path / "components_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "components_facade.cpp"), "-o", out, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    return out


@pytest.mark.parametrize("solid", [False, True])
def test_facade_matches_python(gpu, tmp_path, solid):
    exe = build_facade_program(tmp_path)
    v, t = vx_scenes.torus()
    obj = tmp_path / "t.obj"
    vx_scenes.write_obj(str(obj), v, t)
    vs = F(0.05)
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), vs, gpu.GRID_BOOL, solid=solid)
    for c in CONN:
        out = tmp_path / ("f%d.bin" % c)
        r = subprocess.run([exe, str(obj), repr(float(vs)), str(out), str(c)] + (["solid"] if solid else []), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        lab, k = g.components(c)
        s = g.component_stats(c)
        one = np.uint32(k).tobytes() + lab.tobytes() + s.tobytes()
        assert out.read_bytes() == one * 3


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


@pytest.mark.parametrize("grid", ["bool", "vec"])
@pytest.mark.parametrize("connectivity", [None, 26])
def test_cli_components(gpu, tmp_path, grid, connectivity):
    v, t = vx_scenes.soup(3000)
    obj = tmp_path / "s.obj"
    vx_scenes.write_obj(str(obj), v, t)
    f = tmp_path / "c.csv"
    r = run_cli([str(obj), "0.02", "--grid", grid, "--solid", "--components", str(f)] + (["--connectivity", str(connectivity)] if connectivity else []))
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.02), gpu.GRID_BOOL, solid=True)
    s = g.component_stats(connectivity or 6)
    lines = f.read_text().splitlines()
    assert lines[0] == "label,cells,minx,miny,minz,maxx,maxy,maxz" and len(lines) == len(s) + 1
    got = np.array([[int(x) for x in ln.split(",")] for ln in lines[1:]], dtype=np.int64).reshape(-1, 8)
    assert np.array_equal(got[:, 0], np.arange(1, len(s) + 1))
    assert np.array_equal(got[:, 1], s["cells"]) and np.array_equal(got[:, 2:5], s["min"]) and np.array_equal(got[:, 5:8], s["max"])
    assert ("[voxhip] components: %d" % len(s)) in r.stdout.splitlines()


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--bench", "2"], ["--connectivity", "18"]])
def test_cli_components_refusals(gpu, tmp_path, extra):
    v, t = vx_scenes.cube()
    obj = tmp_path / "c.obj"
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--components", str(tmp_path / "c.csv")] + extra)
    assert r.returncode != 0 and ("--components" in r.stdout or "--connectivity" in r.stdout)
