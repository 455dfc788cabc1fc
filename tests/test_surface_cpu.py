"""CPU tests of the surface mesh: the numpy restatement (tests/surface_ref.py) against a per-cell loop, the 2x2x2 rule, closure,
orientation and the exact enclosed volume, the cross-compiled library's exports and NULL-grid check, and the CLI's refusals of --surface
(all of them run before any device is touched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import surface_ref as sr
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
F = np.float32

# every size from 1 to 9 on every axis
DIMS = [(a, (a * 4) % 9 + 1, (a * 7) % 9 + 1) for a in range(1, 10)]
DIMS += [(z, x, y) for (x, y, z) in DIMS] + [(y, z, x) for (x, y, z) in DIMS]
DENSITIES = (0.0, 0.08, 0.5, 1.0)


def random_cells(dims, p, seed):
    X, Y, Z = dims
    return np.random.default_rng(seed).random((Z, Y, X)) < p


@pytest.mark.parametrize("dims", DIMS)
def test_restatement_matches_per_cell_loop(dims):
    for k, p in enumerate(DENSITIES):
        cells = random_cells(dims, p, sum(dims) * 13 + k)
        org, vs = (0.25, -1.5, 3.0), F(0.37)
        v, t = sr.surface(cells, org, vs)
        bv, bt = sr.brute(cells, org, vs)
        assert v.dtype == np.float32 and t.dtype == np.int32
        assert v.tobytes() == bv.tobytes() and t.tobytes() == bt.tobytes(), (dims, p)


@pytest.mark.parametrize("dims", DIMS[::3] + [(16, 16, 16), (33, 5, 7)])
def test_used_points_follow_the_2x2x2_rule(dims):
    for k, p in enumerate(DENSITIES):
        cells = random_cells(dims, p, 7 + k)
        used, tris, _, _ = sr.surface_lattice(cells)
        assert np.array_equal(used, sr.mixed_corners(cells)), (dims, p)
        assert np.array_equal(np.unique(tris), np.arange(len(used))) or len(used) == 0


def lattice_tris(cells):
    Z, Y, X = cells.shape
    used, tris, cell, d = sr.surface_lattice(cells)
    ijk = sr.lattice_ijk(used, (X, Y, Z))
    return ijk, tris, cell, d


@pytest.mark.parametrize("seed", range(6))
def test_closed_and_oriented(seed):
    rng = np.random.default_rng(seed)
    dims = tuple(int(x) for x in rng.integers(1, 12, 3))
    cells = random_cells(dims, rng.random(), seed)
    X, Y, Z = dims
    ijk, tris, cell, d = lattice_tris(cells)
    # every directed edge is balanced by its reverse
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    fwd = np.sort(e[:, 0] * (1 << 32) + e[:, 1])
    rev = np.sort(e[:, 1] * (1 << 32) + e[:, 0])
    assert np.array_equal(fwd, rev)
    # every normal is e_d, and the cell it points into is empty or outside
    p = ijk[tris]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    dd = np.repeat(d, 2)
    assert np.array_equal(n, sr.DIRS[dd])
    c = np.repeat(cell, 2)
    xyz = np.stack([c % X, (c // X) % Y, c // (X * Y)], axis=-1) + sr.DIRS[dd]
    inside = ((xyz >= 0) & (xyz < np.array([X, Y, Z]))).all(axis=1)
    assert not cells[xyz[inside, 2], xyz[inside, 1], xyz[inside, 0]].any()
    assert cells[(c // (X * Y)), (c // X) % Y, c % X].all()


def signed_volume6(ijk, tris):
    p = ijk[tris].astype(np.int64)
    return int(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum())


@pytest.mark.parametrize("seed", range(8))
def test_enclosed_volume_random(seed):
    rng = np.random.default_rng(100 + seed)
    dims = tuple(int(x) for x in rng.integers(1, 20, 3))
    cells = random_cells(dims, rng.random(), seed)
    ijk, tris, _, _ = lattice_tris(cells)
    assert signed_volume6(ijk, tris) == 6 * int(cells.sum())


@pytest.mark.parametrize("name", ["spiral_maze", "holed_box", "nested", "torus"])
def test_enclosed_volume_of_scene_shapes(name):
    """The spiral maze's mask as it is; the meshes as the cells that hold one of their vertices on a 23^3 grid over their box."""
    if name == "spiral_maze":
        cells = vx_scenes.spiral_maze(24)
    else:
        v, _ = {"holed_box": lambda: vx_scenes.holed_box(0.3), "nested": vx_scenes.nested_shells, "torus": vx_scenes.torus}[name]()
        lo, hi = v.min(axis=0), v.max(axis=0)
        n = 23
        cells = np.zeros((n, n, n), bool)
        idx = np.clip(((v - lo) / np.maximum(hi - lo, 1e-9) * (n - 1)).round().astype(int), 0, n - 1)
        cells[idx[:, 2], idx[:, 1], idx[:, 0]] = True
    assert cells.any()
    ijk, tris, _, _ = lattice_tris(cells)
    assert signed_volume6(ijk, tris) == 6 * int(cells.sum())


def test_empty_full_and_materials():
    cells = np.zeros((3, 4, 5), bool)
    v, t = sr.surface(cells, (0, 0, 0), F(1))
    assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = sr.surface(~cells, (0, 0, 0), F(1))
    assert len(v) == 2 * (6 * 5 + 6 * 4 + 5 * 4) - 4 * (6 + 5 + 4) + 8  # the lattice points of the box's surface
    assert len(t) == 2 * 2 * (5 * 4 + 5 * 3 + 4 * 3)
    assert (v.min(axis=0) == F(0)).all()
    cells = np.zeros((1, 1, 3), bool)
    cells[0, 0, [0, 2]] = True
    v, t, m = sr.surface(cells, (0, 0, 0), F(0.5), cell_ids=np.array([4, 9], np.int16))
    assert m.dtype == np.int32 and len(m) == len(t) == 24 and (m[:12] == 4).all() and (m[12:] == 9).all()


def test_positions_are_cell_minimum_corners():
    ijk = np.array([[0, 0, 0], [3, 1, 2], [7, 7, 7]], np.int64)
    org, vs = (0.1, -2.0, 5.5), F(0.3)
    p = sr.positions(ijk, org, vs)
    half = vs * F(0.5)
    for r, (i, j, k) in enumerate(ijk):
        for a, c in enumerate((i, j, k)):
            assert p[r, a] == (F(org[a]) + ((F(c) + F(0.5)) * vs)) - half


def test_library_exports_the_surface_entry_points(vx):
    L = ctypes.CDLL(vx.LIB_PATH)
    for n in ("vx_grid_surface_device", "vx_grid_surface", "vx_grid_surface_mesh"):
        assert hasattr(L, n) and n in vx.SYMBOLS, n


def test_null_grid_is_invalid(vx):
    L = vx.lib()
    v = np.full(12, 7.0, np.float32)
    t = np.full(12, 5, np.int32)
    nv, nt = ctypes.c_uint64(3), ctypes.c_uint64(4)
    assert L.vx_grid_surface(None, v.ctypes.data, 4, t.ctypes.data, 4, None, ctypes.byref(nv), ctypes.byref(nt)) == 1
    assert L.vx_grid_surface_device(None, v.ctypes.data, 4, t.ctypes.data, 4, None, ctypes.byref(nv), ctypes.byref(nt)) == 1
    assert L.vx_grid_surface(None, None, 0, None, 0, None, None, None) == 1
    h = ctypes.c_void_p()
    assert L.vx_grid_surface_mesh(None, 0, ctypes.byref(h)) == 1
    assert (v == 7.0).all() and (t == 5).all() and h.value is None


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--bench", "2"], ["--grid", "vec", "--materials"]])
def test_cli_surface_refusals(built, tmp_path, extra):
    obj = tmp_path / "c.obj"
    v, t = vx_scenes.cube()
    vx_scenes.write_obj(str(obj), v, t)
    out = tmp_path / "s.obj"
    r = run_cli([str(obj), "0.25", "--surface", str(out)] + extra)
    assert r.returncode == 2 and "--surface writes the boundary mesh of one grid on one device" in r.stdout, r.stdout
    assert not out.exists()
