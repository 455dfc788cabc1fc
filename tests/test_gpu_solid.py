"""GPU tests of solid voxelization (VX_VOXELIZE_SOLID, vx_grid_fill_interior, vx_grid_interior): the bitmask S | H, the lists, counts,
materials, rays and frames of a solid grid against the oracle's surface outputs and the numpy restatement of the fill (tests/solid_ref.py)."""
import re

import numpy as np
import pytest

import oracle
import solid_ref
import vx_scenes
from test_gpu_mesh_trace import run_cli
from test_gpu_render import assert_lsb, read_ppm

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG = 1


def scene(name):
    if name == "torus":
        return vx_scenes.torus()
    if name == "nested":
        return vx_scenes.nested_shells()
    if name == "box_wide_hole":
        return vx_scenes.holed_box(0.6)
    if name == "box_narrow_hole":
        return vx_scenes.holed_box(0.05)
    return vx_scenes.scene(name)


# (scene, voxel size, is H expected to be empty)
# (the axis-aligned cube's faces lie on the grid's last cell planes, where the conservative surface leaves them open: H = {})
CASES = [("cube", 0.25, True), ("cube", 2.0 / 64, True), ("rotcube", 0.09, False), ("blob70k", 2.0 / 64, False), ("blob70k", 2.0 / 97, False),
         ("torus", 0.05, False), ("nested", 0.07, False), ("box_wide_hole", 0.1, True), ("box_narrow_hole", 0.1, False), ("atrium262k", 32.0 / 128, None)]


def expected(v, t, vs, sat):
    ow, calls, gi = oracle.build_bool(v, t, vs, threads=0, sat=sat)
    sw, hw, nh = solid_ref.fill(ow, gi["dim"])
    return ow, calls, gi, sw, hw, nh


def check_solid(gpu, g, kind, v, t, vs, sat, exp):
    ow, calls, gi, sw, hw, nh = exp
    d = g.describe()
    assert d["dim"] == gi["dim"] and d["triangles"] == len(t)
    assert np.array_equal(g.bitmask(), sw), "bitmask: %d differing words" % int((g.bitmask() != sw).sum())
    assert g.interior() == nh
    assert d["occupied"] == int(np.unpackbits(sw.view(np.uint8)).sum())
    if kind == gpu.GRID_VEC:
        ov = solid_ref.solid_vec(oracle.build_vec(v, t, vs, threads=0, sat=sat), hw, gi, vs)
        assert g.aabbs().tobytes() == ov.tobytes()
        assert d["set_calls"] == len(ov) and g.memory_bytes() == 24 * len(ov)
    else:
        assert g.aabbs().tobytes() == oracle.bool_aabbs(sw, gi, vs).tobytes()
        assert d["set_calls"] == calls + nh
        n = int(np.prod(gi["dim"]))
        assert g.memory_bytes() == (4 * ((n + 31) // 32) if kind == gpu.GRID_BOOL else 28 * n)


@pytest.mark.parametrize("name,vs,empty", CASES)
@pytest.mark.parametrize("sat", [0, 1])
def test_solid_parity(gpu, name, vs, empty, sat):
    v, t = scene(name)
    vs = F(vs)
    exp = expected(v, t, vs, sat)
    if empty is not None:
        assert (exp[5] == 0) == empty, "scene %s: |H| = %d" % (name, exp[5])
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, vs, kind, sat_variant=sat, solid=True)
        check_solid(gpu, g, kind, v, t, vs, sat, exp)


def test_solid_blob_256(gpu):
    v, t = vx_scenes.blob()
    vs = F(2.0 / 256)
    exp = expected(v, t, vs, 0)
    assert exp[2]["dim"] == (256, 256, 256) and exp[5] > 1_000_000
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, vs, kind, solid=True)
        check_solid(gpu, g, kind, v, t, vs, 0, exp)
        assert g.fill_rounds() >= 2


def thin_box(length=70000.3, side=5.7):
    """a closed box far longer along x than 65535 cells at voxel size 1 (the wide path of the voxelizer and the ray kernel)"""
    v, t = vx_scenes.cube(0.5, center=(0.5, 0.5, 0.5))
    return (v * np.float32([length, side, side])).astype(np.float32), t


def test_solid_wide_axis(gpu):
    v, t = thin_box()
    vs = F(1.0)
    exp = expected(v, t, vs, 0)
    assert exp[2]["dim"][0] > 65535 and exp[5] > 0
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        check_solid(gpu, gpu.Grid.voxelize(mesh, vs, kind, solid=True), kind, v, t, vs, 0, exp)


@pytest.mark.parametrize("size", [(5.7, 70000.3, 5.7), (40.3, 5.7, 50000.3), (127.6, 3.5, 9000.2)])
def test_solid_long_column_axis(gpu, size):
    """A closed thin box whose long axis is y or z: the column scans run over thousands of chunks (dozens of 64-chunk steps of the carry
    scan per column); X % 32 != 0 and X % 32 == 0 rows."""
    v, t = vx_scenes.cube(0.5, center=(0.5, 0.5, 0.5))
    v = (v * np.float32(size)).astype(np.float32)
    vs = F(1.0)
    exp = expected(v, t, vs, 0)
    assert max(exp[2]["dim"][1:]) > 8000 and exp[5] > 0
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        check_solid(gpu, gpu.Grid.voxelize(mesh, vs, kind, solid=True), kind, v, t, vs, 0, exp)


@pytest.mark.parametrize("axis", [1, 0])
def test_fill_interior_long_channel(gpu, axis):
    """A solid block crossed by a one-cell channel that opens on the boundary and runs almost the whole length of a long y or z axis (the
    exterior reaches its end only through the column scan's carries), beside a closed cavity of the same length (interior)."""
    L = 6000
    cells = np.ones((L, 9, 37), bool)          # [z, y, x]
    cells[0:L - 10, 4, 18] = False             # the channel, open at z = 0
    cells[5:L - 5, 3:6, 8:11] = False          # the cavity
    if axis == 1:
        cells = np.ascontiguousarray(cells.transpose(1, 0, 2))   # the long axis becomes y
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        g, nh = check_fill(gpu, cells, kind)
        assert nh == (L - 10) * 9


# ---- vx_grid_fill_interior on masks from setVoxel and from outside ---------------------------------------------------------------------
def write_mask(g, words):
    import torch
    n = len(words)

    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (g.bitmask_device_ptr(mutable=True), False), "version": 3, "strides": None}
    torch.as_tensor(View(), device="cuda").copy_(torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda())
    torch.cuda.synchronize()


def check_fill(gpu, cells, kind, vs=F(0.5), origin=(0.25, -1.0, 3.0)):
    Z, Y, X = cells.shape
    words = solid_ref.pack(cells)
    g = gpu.Grid.create(kind, X, Y, Z, vs, origin)
    write_mask(g, words)
    g.refresh()
    before = g.aabbs() if kind == gpu.GRID_VEC else None
    n = g.fill_interior()
    sw, hw, nh = solid_ref.fill(words, (X, Y, Z))
    assert n == nh == g.interior()
    assert np.array_equal(g.bitmask(), sw)
    gi = dict(dim=(X, Y, Z), bmin=np.array(origin, np.float32))
    d = g.describe()
    assert d["set_calls"] == nh and d["occupied"] == int(np.unpackbits(sw.view(np.uint8)).sum())
    if kind == gpu.GRID_VEC:
        assert len(before) == 0 and g.aabbs().tobytes() == oracle.bool_aabbs(hw, gi, vs).tobytes()
    else:
        assert g.aabbs().tobytes() == oracle.bool_aabbs(sw, gi, vs).tobytes()
    return g, nh


def test_fill_interior_spiral_maze(gpu):
    cells = vx_scenes.spiral_maze(96)
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        g, nh = check_fill(gpu, cells, kind)
        assert nh == 64                    # only the closed core: every gap between the shells is reached from outside
        assert g.fill_rounds() >= 15       # the way in turns at every shell


@pytest.mark.parametrize("dims,density,seed", [((97, 61, 45), 0.3, 1), ((64, 40, 33), 0.33, 2), ((33, 34, 35), 0.45, 3), ((128, 3, 9), 0.4, 4),
                                               ((5, 70, 6), 0.5, 5), ((2, 40, 40), 0.5, 6), ((31, 31, 1), 0.2, 7)])
def test_fill_interior_random_masks(gpu, dims, density, seed):
    rng = np.random.default_rng(seed)
    X, Y, Z = dims
    cells = rng.random((Z, Y, X)) < density
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        check_fill(gpu, cells, kind)


def test_fill_interior_after_set_voxel(gpu):
    """setVoxel on a hollow 6^3 shell of a 10^3 grid, then the fill: 4^3 interior cells appended to the Vec list in ascending order."""
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        g = gpu.Grid.create(kind, 10, 10, 10, F(0.25))
        cells = np.zeros((10, 10, 10), bool)
        for z in range(2, 8):
            for y in range(2, 8):
                for x in range(2, 8):
                    if min(x, y, z) == 2 or max(x, y, z) == 7:
                        g.set_voxel(x, y, z)
                        cells[z, y, x] = True
        before = g.aabbs()
        assert g.fill_interior() == 64 and g.describe()["set_calls"] == len(before) + 64
        sw, hw, _ = solid_ref.fill(solid_ref.pack(cells), (10, 10, 10))
        assert np.array_equal(g.bitmask(), sw)
        gi = dict(dim=(10, 10, 10), bmin=np.zeros(3, np.float32))
        if kind == gpu.GRID_VEC:
            assert g.aabbs().tobytes() == before.tobytes() + oracle.bool_aabbs(hw, gi, F(0.25)).tobytes()
        assert g.fill_interior() == 0     # a second fill finds nothing left


# ---- materials ---------------------------------------------------------------------------------------------------------------------
def _materials(gpu, n, seed):
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=gpu.MATERIAL)
    recs["diffuse"] = rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32)
    recs["ambient"] = 0.05
    recs["illum"] = 2
    return recs


@pytest.mark.parametrize("name,vs,with_default", [("blob70k", 2.0 / 64, False), ("blob70k", 2.0 / 64, True), ("torus", 0.05, False), ("rotcube", 0.09, True)])
def test_solid_materials(gpu, name, vs, with_default):
    """Surface voxels and calls keep the ids of a surface build; the interior carries MaterialObj{}, appended to the table when no triangle
    used it (value 0 of oracle.material_ids)."""
    v, t = scene(name)
    vs = F(vs)
    recs = _materials(gpu, 3, 7)
    ids = (np.arange(len(t)) % 3).astype(np.int32)
    if with_default:
        ids[::5] = -1                   # faces without a material: MaterialObj{} is used by triangles too
    mesh = gpu.Mesh.from_arrays(v, t)
    mesh.set_materials(recs, ids)
    tv = np.where(ids >= 0, ids + 1, 0).astype(np.int32)   # value ids: 0 = MaterialObj{}, then the three distinct records
    ow, calls, gi, sw, hw, nh = expected(v, t, vs, 0)
    assert nh > 0
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, vs, kind, materials=True, solid=True)
        mats, mid = g.materials()
        if kind == gpu.GRID_VEC:
            oids, order = oracle.material_ids(v, t, vs, tv, 4, per_call=True, ncalls=len(oracle.build_vec(v, t, vs)))
            exp_ids, exp_order = solid_ref.solid_material_ids_vec(oids, nh, order)
        else:
            oids, order = oracle.material_ids(v, t, vs, tv, 4)
            exp_ids, exp_order = solid_ref.solid_material_ids_bool(oids, ow, hw, gi["dim"], order)
        assert np.array_equal(mid, exp_ids), "kind %d" % kind
        assert len(mats) == len(exp_order) and len(mid) == len(g.aabbs())
        d = exp_order.index(0)
        assert mats[d]["diffuse"].tolist() == [1, 1, 0] and mats[d]["illum"] == 0
        if not with_default:
            assert d == len(exp_order) - 1     # appended by the second loop


# ---- rays and frames ---------------------------------------------------------------------------------------------------------------
def _dilate(cells, r):
    out = cells.copy()
    for axis in range(3):
        acc = out.copy()
        for k in range(1, r + 1):
            acc[(slice(None),) * axis + (slice(k, None),)] |= out[(slice(None),) * axis + (slice(None, -k),)]
            acc[(slice(None),) * axis + (slice(None, -k),)] |= out[(slice(None),) * axis + (slice(k, None),)]
        out = acc
    return out


def test_rays_from_inside(gpu):
    """Rays from the centres of interior cells at least three cells away from the surface: on the solid grid they stop within one voxel
    diagonal (bit-equal to the brute force over the solid list), on the surface grid they travel more than two voxels to the wall."""
    v, t = vx_scenes.blob()
    vs = F(2.0 / 64)
    ow, calls, gi, sw, hw, nh = expected(v, t, vs, 0)
    dim = gi["dim"]
    s = solid_ref.unpack(ow, dim)
    h = solid_ref.unpack(hw, dim)
    deep = np.argwhere(h & ~_dilate(s, 3))
    assert len(deep) > 100
    rng = np.random.default_rng(3)
    pick = deep[rng.choice(len(deep), min(4000, len(deep)), replace=False)]
    o = gi["bmin"] + (pick[:, ::-1].astype(np.float32) + F(0.5)) * vs
    d = rng.normal(size=(len(pick), 3)).astype(np.float32)
    rays = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    mesh = gpu.Mesh.from_arrays(v, t)
    solid = gpu.Grid.voxelize(mesh, vs, solid=True)
    surf = gpu.Grid.voxelize(mesh, vs)
    tt, pp, _ = solid.trace(rays)
    ot, op = oracle.trace_brute(oracle.bool_aabbs(sw, gi, vs), rays)
    assert np.array_equal(tt, ot) and np.array_equal(pp, op)
    assert (tt > 0).all() and (tt <= vs * np.sqrt(3.0)).all()
    ts, _, _ = surf.trace(rays)
    assert (ts > 2 * vs).all()


def test_solid_frame_matches_cli(gpu, tmp_path):
    """A Renderer frame of a solid Bool grid against voxilizer --solid --render (host shading of the same grid) within 1 LSB."""
    v, t = vx_scenes.holed_box(0.05)
    obj = tmp_path / "box.obj"
    vx_scenes.write_obj(str(obj), v, t)
    W, H = 320, 180
    ppm, cam = tmp_path / "cli.ppm", tmp_path / "cam.bin"
    r = run_cli([str(obj), "0.1", "--solid", "--render", str(ppm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)])
    assert r.returncode == 0, r.stdout
    mesh = gpu.Mesh.load_obj(str(obj))
    g = gpu.Grid.voxelize(mesh, F(0.1), solid=True)
    m = re.search(r"\[voxhip\] solid: (\d+) interior voxels filled", r.stdout)
    assert m and int(m.group(1)) == g.interior() > 0, r.stdout
    cm = np.fromfile(cam, np.float32)
    rd = gpu.Renderer(g)
    out = rd.render_host((cm[:16], cm[16:], W, H), None, want=("rgba",))
    img = out["rgba"].reshape(W * H, 4)[:, :3]
    ref = read_ppm(ppm, W, H)
    assert_lsb(img, ref, "Renderer vs voxilizer --solid --render")
    assert len(np.unique(ref, axis=0)) > 4
    rd.free()


@pytest.mark.parametrize("grid", ["bool", "aabbstruct", "vec"])
def test_cli_solid_line(gpu, tmp_path, grid):
    v, t = vx_scenes.nested_shells()
    obj = tmp_path / "n.obj"
    vx_scenes.write_obj(str(obj), v, t)
    plain = run_cli([str(obj), "0.07", "--grid", grid])
    solid = run_cli([str(obj), "0.07", "--grid", grid, "--solid"])
    assert plain.returncode == 0 and solid.returncode == 0, solid.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(0.07), {"bool": gpu.GRID_BOOL, "aabbstruct": gpu.GRID_AABBSTRUCT, "vec": gpu.GRID_VEC}[grid], solid=True)
    assert "[voxhip] solid: %d interior voxels filled" % g.interior() in solid.stdout
    keep = lambda out: [ln for ln in out.splitlines() if not re.search(r"took \d+ms|Mvoxels/s|Total usage|solid:", ln)]
    assert keep(plain.stdout) == keep(solid.stdout)


# ---- handle reuse and errors -------------------------------------------------------------------------------------------------------
def test_handle_reuse(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        big, small = F(2.0 / 128), F(2.0 / 40)
        g = gpu.Grid.voxelize(mesh, big, kind, solid=True)
        assert g.interior() > 0
        g.revoxelize(mesh, big)                  # solid, then surface: a fresh surface build
        fresh = gpu.Grid.voxelize(mesh, big, kind)
        assert np.array_equal(g.bitmask(), fresh.bitmask()) and g.aabbs().tobytes() == fresh.aabbs().tobytes()
        assert g.interior() == 0 and g.describe()["set_calls"] == fresh.describe()["set_calls"]
        g.revoxelize(mesh, big, solid=True)
        g.revoxelize(mesh, small, solid=True)   # a smaller solid grid after a larger one: nothing stale
        exp = expected(v, t, small, 0)
        check_solid(gpu, g, kind, v, t, small, 0, exp)
        g.revoxelize(mesh, big, solid=True)
        n0 = gpu.device_allocations()
        for _ in range(3):
            g.revoxelize(mesh, big, solid=True)
        assert gpu.device_allocations() == n0
        check_solid(gpu, g, kind, v, t, big, 0, expected(v, t, big, 0))


def test_errors_keep_previous_build(gpu):
    import ctypes as C
    v, t = vx_scenes.blob()
    vs = F(2.0 / 64)
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, vs, solid=True)
    w0, n0, a0 = g.bitmask(), g.interior(), g.aabbs()
    nwords = g.describe()["num_words"]
    for kw in (dict(words=(0, nwords // 2)), dict(shard=(0, 2)), dict(shard=(1, 2)), dict(tris=(0, len(t))), dict(tris=(0, 10))):
        with pytest.raises(gpu.VxError) as ei:
            g.revoxelize(mesh, vs, solid=True, **kw)
        assert ei.value.status == INVALID_ARG, kw
        assert np.array_equal(g.bitmask(), w0) and g.interior() == n0 and g.aabbs().tobytes() == a0.tobytes()
    m = gpu.Multi(mesh, [0, 0])
    o = gpu.VoxelizeOpts()
    o.flags = gpu.VOXELIZE_SOLID
    st = gpu.lib().vx_multi_voxelize(m.h, F(vs), C.byref(o), 0)
    assert st == INVALID_ARG
    m.free()
    assert gpu.lib().vx_grid_interior(None, None) == INVALID_ARG


def test_default_build_unchanged_kernels(gpu):
    """A surface build queues no kernel of the fill, and its bitmask is the oracle's."""
    v, t = vx_scenes.blob()
    vs = F(2.0 / 64)
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, vs)
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any("solid" in n for n in names), names
    assert np.array_equal(g.bitmask(), oracle.build_bool(v, t, vs)[0]) and g.interior() == 0
