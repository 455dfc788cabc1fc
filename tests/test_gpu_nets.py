"""GPU tests of the surface-nets mesh (vx_grid_surface_smooth*): every output is compared whole, bit for bit, with the restatement
(tests/nets_ref.py) of the GPU's own bitmask, host and device variants alike; triangles and ids are those of vx_grid_surface."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nets_ref as nr
import surface_ref as sr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY, UNSUPPORTED = 1, 8, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
ORG = (0.25, -1.0, 3.0)
PARAMS = [(1.0, 0.0), (0.5, 0.0), (0.5, -0.53)]


def masked_grid(gpu, cells, kind=None, vs=F(0.37)):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, vs, ORG)
    write_mask(g, sr.pack(cells))
    g.refresh()
    return g


def same(got, want, what=""):
    names = ("verts", "tris", "third", "fourth")
    assert len(got) == len(want)
    for a, b, name in zip(got, want, names):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s %s differ at %d entries" % (what, name, int((a != b).sum()))


def check(gpu, g, iterations, lam, mu, materials=False, normals=True, device=True, cells=None):
    """host and device arrays of the grid against the restatement of its own bitmask"""
    d = g.describe()
    if cells is None:
        cells = sr.unpack(g.bitmask(), d["dim"])
    ids = g.materials()[1] if materials else None
    want = nr.surface_smooth(cells, d["origin"], F(d["voxel_size"]), iterations, lam, mu, cell_ids=ids, with_normals=normals)
    same(g.surface_smooth(iterations, lam, mu, materials=materials, normals=normals), want, "host")
    if device:
        import torch
        dev = g.surface_smooth_device(iterations, lam, mu, materials=materials, normals=normals)
        torch.cuda.synchronize()
        same(dev, want, "device")
    return cells, want


def random_cells(dims, density):
    X, Y, Z = dims
    return np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density


DIMS = [(1, 1, 1), (5, 3, 2), (31, 2, 2), (32, 1, 1), (33, 3, 3), (63, 5, 4)]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95, 1.0])
def test_small_dimensions(gpu, dims, density):
    cells = random_cells(dims, density)   # (density 1.0: the fully occupied grid)
    g = masked_grid(gpu, cells)
    for it in (0, 1, 2, 7):
        for lam, mu in PARAMS:
            check(gpu, g, it, lam, mu, normals=(it != 1), cells=cells)
    # tri is bit-equal to vx_grid_surface's on the same grid
    assert g.surface_smooth(2)[1].tobytes() == g.surface()[1].tobytes()


@pytest.mark.parametrize("dims", DIMS)
def test_occupied_borders(gpu, dims):
    X, Y, Z = dims
    cells = np.zeros((Z, Y, X), bool)
    cells[0], cells[-1], cells[:, 0], cells[:, -1], cells[:, :, 0], cells[:, :, -1] = (True,) * 6
    if min(dims) > 2:
        cells[Z // 2, Y // 2, X // 2] = True
    g = masked_grid(gpu, cells)
    for it, (lam, mu) in ((0, PARAMS[2]), (7, PARAMS[2]), (2, PARAMS[0])):
        check(gpu, g, it, lam, mu, cells=cells)


def test_non_manifold_contacts(gpu):
    edge = np.zeros((1, 2, 2), bool)
    edge[0, 0, 0] = edge[0, 1, 1] = True
    corner = np.zeros((2, 2, 2), bool)
    corner[0, 0, 0] = corner[1, 1, 1] = True
    for cells, (V, T) in ((edge, (14, 24)), (corner, (15, 24))):
        g = masked_grid(gpu, cells)
        for it in (0, 1, 2, 7):
            for lam, mu in PARAMS:
                _, want = check(gpu, g, it, lam, mu, cells=cells)
                assert (len(want[0]), len(want[1])) == (V, T)


def test_ball_64(gpu):
    c = (np.arange(64) + 0.5) - 32.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    cells = x * x + y * y + z * z <= 27.3 ** 2
    g = masked_grid(gpu, cells, vs=F(1))
    for it, (lam, mu) in ((0, PARAMS[2]), (1, PARAMS[1]), (7, PARAMS[2]), (2, PARAMS[0])):
        _, want = check(gpu, g, it, lam, mu, cells=cells)
    v, _, n = want
    centre = np.array(ORG) + 32.0
    assert ((n * (v - centre)).sum(axis=1) > 0).all()


def test_large_i(gpu):
    cells = np.zeros((2, 2, 70000), bool)
    cells[0, 0, 69999] = cells[1, 1, 69998] = cells[0, 1, 69990] = cells[1, 0, 65537] = cells[0, 0, 0] = True
    cells[:, :, 69993:69996] = True
    g = masked_grid(gpu, cells, vs=F(0.013))
    for it, (lam, mu) in ((0, PARAMS[2]), (7, PARAMS[2])):
        check(gpu, g, it, lam, mu, cells=cells)


def scene(name):
    return {"torus": vx_scenes.torus, "nested": vx_scenes.nested_shells}[name]()


@pytest.mark.parametrize("solid", [False, True])
def test_mesh_built_grids(gpu, solid):
    v, t = scene("torus")
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind, it, (lam, mu) in ((gpu.GRID_BOOL, 7, PARAMS[2]), (gpu.GRID_AABBSTRUCT, 2, PARAMS[0]), (gpu.GRID_VEC, 1, PARAMS[1])):
        g = gpu.Grid.voxelize(mesh, F(0.05), kind, solid=solid)
        cells, want = check(gpu, g, it, lam, mu)
        assert cells.any() and len(want[1]) > 0
        assert want[1].tobytes() == g.surface()[1].tobytes()


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


@pytest.mark.parametrize("normals", [False, True])
def test_materials(gpu, normals):
    mesh = material_mesh(gpu)
    vs = F(2.0 / 48)
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT):
        g = gpu.Grid.voxelize(mesh, vs, kind, materials=True)
        _, want = check(gpu, g, 2, 0.5, -0.53, materials=True, normals=normals)
        assert len(np.unique(want[2])) > 1
        bv, bt, bm = g.surface(materials=True)
        assert want[1].tobytes() == bt.tobytes() and want[2].tobytes() == bm.tobytes()
        check(gpu, g, 2, 0.5, -0.53, materials=False, normals=normals, device=False)


def _smooth(gpu, it=2, lam=0.5, mu=-0.53):
    return gpu.Smooth(it, lam, mu)


def test_argument_errors_write_nothing(gpu):
    import torch
    cells = random_cells((7, 6, 5), 0.3)
    g = masked_grid(gpu, cells)
    want = nr.surface_smooth(cells, ORG, F(0.37), 2, with_normals=True)
    V, T = len(want[0]), len(want[1])
    L = gpu.lib()
    nv, nt = ctypes.c_uint64(), ctypes.c_uint64()
    ok = _smooth(gpu)
    assert L.vx_grid_surface_smooth(g.h, ctypes.byref(ok), None, 0, None, 0, None, None, ctypes.byref(nv), ctypes.byref(nt)) == 0
    assert (nv.value, nt.value) == (V, T)
    hv = np.full(3 * V, 9.5, np.float32)
    hn = np.full(3 * V, 8.5, np.float32)
    ht = np.full(3 * T, -3, np.int32)
    hm = np.full(T, -4, np.int32)
    dv = torch.full((3 * V,), 9.5, device="cuda")
    dn = torch.full((3 * V,), 8.5, device="cuda")
    dt = torch.full((3 * T,), -3, dtype=torch.int32, device="cuda")

    def host(sp, xyz=hv.ctypes.data, vcap=V, tri=ht.ctypes.data, tcap=T, mat=None, grid=g):
        return L.vx_grid_surface_smooth(grid.h if grid else None, ctypes.byref(sp) if sp is not None else None, xyz, vcap, tri, tcap, mat,
                                        hn.ctypes.data, ctypes.byref(nv), ctypes.byref(nt))

    def dev(sp, xyz=dv.data_ptr(), vcap=V, tri=dt.data_ptr(), tcap=T, grid=g):
        return L.vx_grid_surface_smooth_device(grid.h if grid else None, ctypes.byref(sp) if sp is not None else None, xyz, vcap, tri, tcap, None,
                                               dn.data_ptr(), ctypes.byref(nv), ctypes.byref(nt))

    bad = [_smooth(gpu, 1025), _smooth(gpu, 2, float("nan")), _smooth(gpu, 2, 1.5), _smooth(gpu, 2, 0.5, 0.1),
           _smooth(gpu, 2, 0.5, float("-inf")), None]
    for call in (host, dev):
        for sp in bad:
            assert call(sp) == INVALID_ARG
        # a bad vx_smooth comes before the capacity check
        assert call(bad[0], vcap=V - 1) == INVALID_ARG
        assert call(ok, grid=None) == INVALID_ARG
        assert call(ok, xyz=None) == INVALID_ARG
        assert call(ok, tri=None) == INVALID_ARG
        for caps in ((V - 1, T), (V, T - 1)):
            nv.value = nt.value = 0
            assert call(ok, vcap=caps[0], tcap=caps[1]) == CAPACITY
            assert (nv.value, nt.value) == (V, T)
    # materials: a grid without ids, and a Vec grid
    assert host(ok, mat=hm.ctypes.data) == INVALID_ARG
    cv, ct = vx_scenes.cube()
    vec = gpu.Grid.voxelize(gpu.Mesh.from_arrays(cv, ct), F(0.25), gpu.GRID_VEC)
    assert host(ok, mat=hm.ctypes.data, grid=vec) == UNSUPPORTED
    h = ctypes.c_void_p()
    assert L.vx_grid_surface_smooth_mesh(vec.h, ctypes.byref(ok), 1, 1, ctypes.byref(h)) == UNSUPPORTED and h.value is None
    assert L.vx_grid_surface_smooth_mesh(g.h, ctypes.byref(bad[0]), 0, 1, ctypes.byref(h)) == INVALID_ARG and h.value is None
    assert L.vx_grid_surface_smooth_mesh(g.h, None, 0, 1, ctypes.byref(h)) == INVALID_ARG and h.value is None
    torch.cuda.synchronize()
    assert (hv == 9.5).all() and (hn == 8.5).all() and (ht == -3).all() and (hm == -4).all()
    assert (dv.cpu() == 9.5).all() and (dn.cpu() == 8.5).all() and (dt.cpu() == -3).all()
    # exact capacities write exactly the arrays
    assert host(ok) == 0
    assert hv.tobytes() == want[0].tobytes() and ht.tobytes() == want[1].tobytes() and hn.tobytes() == want[2].tobytes()
    for it, lam, mu in ((1025, 0.5, 0.0), (1, 1.5, 0.0), (1, 0.5, 0.1)):
        with pytest.raises(gpu.VxError):
            g.surface_smooth(it, lam, mu)


def test_failed_build_is_empty_and_ok(gpu):
    import torch
    v, t = vx_scenes.cube()
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, F(0.25))
    with pytest.raises(gpu.VxError):
        g.revoxelize(mesh, F(2.0 / ((1 << 21) + 4096)))
    assert g.describe()["dim"] == (0, 0, 0)
    L = gpu.lib()
    sp = _smooth(gpu)
    hv = np.full(12, 7.0, np.float32)
    ht = np.full(12, 5, np.int32)
    nv, nt = ctypes.c_uint64(3), ctypes.c_uint64(4)
    assert L.vx_grid_surface_smooth(g.h, ctypes.byref(sp), hv.ctypes.data, 4, ht.ctypes.data, 4, None, hv.ctypes.data, ctypes.byref(nv),
                                    ctypes.byref(nt)) == 0
    assert nv.value == 0 and nt.value == 0
    dv = torch.full((12,), 3.0, device="cuda")
    nv.value, nt.value = 3, 4
    assert L.vx_grid_surface_smooth_device(g.h, ctypes.byref(sp), dv.data_ptr(), 4, dv.data_ptr(), 4, None, dv.data_ptr(), ctypes.byref(nv),
                                           ctypes.byref(nt)) == 0
    assert nv.value == 0 and nt.value == 0
    torch.cuda.synchronize()
    assert (hv == 7.0).all() and (ht == 5).all() and (dv.cpu() == 3.0).all()
    vv, tt, nn = g.surface_smooth(normals=True)
    assert vv.shape == (0, 3) and tt.shape == (0, 3) and nn.shape == (0, 3)
    assert g.surface_smooth_mesh(normals=True).num_triangles == 0


def test_non_default_stream(gpu):
    import torch
    v, t = vx_scenes.blob()
    st = torch.cuda.Stream()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 61), gpu.GRID_BOOL, stream=st.cuda_stream)
    with torch.cuda.stream(st):
        dev = g.surface_smooth_device(3, normals=True)
    st.synchronize()
    same(dev, g.surface_smooth(3, normals=True))
    check(gpu, g, 3, 0.5, -0.53, device=False)


def _same_desc(a, b):
    return all((np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]) for k in a)


def test_no_side_effects_on_async_list(gpu):
    mesh = material_mesh(gpu)
    vs = F(2.0 / 48)
    a = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    b = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC, materials=True)
    a.revoxelize(mesh, vs, materials=True, list_async=True)
    b.revoxelize(mesh, vs, materials=True, list_async=True)
    b.surface_smooth(3, normals=True)
    b.surface_smooth_device(3, normals=True)
    assert _same_desc(a.describe(), b.describe()) and np.array_equal(a.bitmask(), b.bitmask())
    assert a.aabbs().tobytes() == b.aabbs().tobytes()
    ma, ia = a.materials()
    mb, ib = b.materials()
    assert ma.tobytes() == mb.tobytes() and ia.tobytes() == ib.tobytes()


def test_repeated_calls_allocate_nothing(gpu):
    g = masked_grid(gpu, random_cells((40, 33, 21), 0.4))
    g.surface_smooth(5, normals=True)
    g.surface_smooth_device(5, normals=True)
    n0, b0 = gpu.device_allocations(), gpu.device_live_blocks()
    for _ in range(3):
        g.surface_smooth(5, normals=True)
        g.surface_smooth_device(5, normals=True)
    assert gpu.device_allocations() == n0, "a repeated call at the same dimensions and parameters allocated"
    assert gpu.device_live_blocks() == b0


def test_default_paths_queue_no_nets_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    rays = vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1)
    g.trace(rays)
    g.surface()
    names = list(gpu.profile_read())
    gpu.profile_reset()
    g.surface_smooth(2, normals=True)
    nets = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any("k_nets" in n for n in names), names
    for k in ("k_nets_init", "k_nets_table", "k_nets_relax", "k_nets_finish", "k_nets_normals", "k_surf_emit", "k_surf_count"):
        assert any(k in n for n in nets), (k, nets)
    assert not any("k_surf_verts" in n for n in nets), nets


def test_smooth_mesh_normals_bvh_and_frame(gpu):
    v, t = vx_scenes.blob()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 24), gpu.GRID_BOOL)
    pv, pt, pn = g.surface_smooth(4, normals=True)
    sm = g.surface_smooth_mesh(4, normals=True)
    hv, ht = sm.host_arrays()
    assert hv.tobytes() == pv.tobytes() and ht.tobytes() == pt.tobytes()
    cn = sm.corner_normals()
    assert cn.shape == (len(pt), 3, 3) and cn.tobytes() == pn[pt].tobytes()
    plain = g.surface_smooth_mesh(4, normals=False)
    assert plain.corner_normals() is None
    assert plain.host_arrays()[0].tobytes() == pv.tobytes()
    bvh, bvh_plain = gpu.Bvh(sm), gpu.Bvh(plain)
    assert bvh.num_triangles == len(pt)
    bv, bt = vx_scenes.cube(half=0.2, center=(3.0, 0.0, 0.0))
    vox = gpu.Grid.voxelize(gpu.Mesh.from_arrays(bv, bt), F(0.1))
    vi, pi = vx_scenes.camera_matrices(eye=(2.5, 2.0, -3.0), ctr=(0.0, 0.0, 0.0), aspect=1.0)
    cam = (vi, pi, 32, 32)
    a = gpu.Renderer(vox, bvh, sm, attributes=True).render_host(cam, want=("rgba", "kind"))
    b = gpu.Renderer(vox, bvh_plain, plain, attributes=True).render_host(cam, want=("rgba", "kind"))
    assert (a["kind"] == 2).sum() > 50 and np.array_equal(a["kind"], b["kind"])
    assert (a["rgba"] != b["rgba"]).any()


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_cli_obj_round_trip(gpu, tmp_path):
    v, t = vx_scenes.torus()
    obj = tmp_path / "t.obj"
    vx_scenes.write_obj(str(obj), v, t)
    out = tmp_path / "s.obj"
    r = run_cli([str(obj), "0.07", "--surface", str(out), "--smooth", "4"])
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.07), gpu.GRID_BOOL)
    pv, pt, pn = g.surface_smooth(4, normals=True)
    back = gpu.Mesh.load_obj(str(out))
    hv, ht = back.host_arrays()
    # %.9g prints a float32 exactly enough to read it back
    assert hv.tobytes() == pv.tobytes() and ht.tobytes() == pt.tobytes()
    assert back.corner_normals().tobytes() == pn[pt].tobytes()
    text = out.read_text()
    assert text.count("\nvn ") == len(pv) and "//" in text
    r = run_cli([str(obj), "0.07", "--surface", str(out), "--smooth", "3:1:0"])
    assert r.returncode == 0, r.stdout
    assert gpu.Mesh.load_obj(str(out)).host_arrays()[0].tobytes() == g.surface_smooth(3, 1.0, 0.0)[0].tobytes()


@pytest.mark.parametrize("args", [["--smooth", "4"], ["--surface", "S", "--smooth", "4", "--grid", "octree"], ["--surface", "S", "--smooth", "2000"],
                                  ["--surface", "S", "--smooth", "4:2:0"], ["--surface", "S", "--smooth", "x"]])
def test_cli_refusals(gpu, tmp_path, args):
    v, t = vx_scenes.cube()
    obj = tmp_path / "c.obj"
    vx_scenes.write_obj(str(obj), v, t)
    out = tmp_path / "s.obj"
    r = run_cli([str(obj), "0.25"] + [str(out) if a == "S" else a for a in args])
    assert r.returncode == 2 and r.stdout.strip(), r.stdout
    assert not out.exists()


def build_facade_program(tmp_path):
    import build as vxbuild
    exe = str(tmp_path / "nets_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "nets_facade.cpp"), "-o", exe, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    return exe


def fnv(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_facade_matches_python(gpu, tmp_path):
    exe = build_facade_program(tmp_path)
    v, t = vx_scenes.torus()
    obj = tmp_path / "t.obj"
    vx_scenes.write_obj(str(obj), v, t)
    r = subprocess.run([exe, str(obj), "0.09", "3", "0.5", "-0.53"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("nets ")]
    assert len(lines) == 3, r.stdout
    mesh = gpu.Mesh.load_obj(str(obj))
    for kind, line in zip((gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC), lines):
        pv, pt, pn = gpu.Grid.voxelize(mesh, F(0.09), kind).surface_smooth(3, 0.5, -0.53, normals=True)
        h = fnv(fnv(fnv(14695981039346656037, pv.tobytes()), pt.tobytes()), pn.tobytes())
        assert line.split() == [str(len(pv)), str(len(pt)), "%016x" % h], (line, len(pv), len(pt))
