"""CPU tests of solid voxelization: the numpy restatement of the fill (tests/solid_ref.py) against scipy's binary_fill_holes and on hand-worked
cases, the closed test scenes, and the CLI's argument errors for --solid."""
import os
import subprocess

import numpy as np
import pytest

import solid_ref
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")


def fill_cells(cells):
    Z, Y, X = cells.shape
    sw, hw, n = solid_ref.fill(solid_ref.pack(cells), (X, Y, Z))
    return solid_ref.unpack(sw, (X, Y, Z)), solid_ref.unpack(hw, (X, Y, Z)), n


@pytest.mark.parametrize("dims", [(97, 61, 45), (64, 40, 33), (33, 34, 35), (5, 70, 6), (128, 3, 9)])
@pytest.mark.parametrize("density", [0.25, 0.31, 0.4])
def test_reference_matches_scipy(dims, density):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100) + dims[0])
    X, Y, Z = dims
    cells = rng.random((Z, Y, X)) < density
    s, h, n = fill_cells(cells)
    exp = nd.binary_fill_holes(cells)
    assert np.array_equal(s, exp) and n == int((exp & ~cells).sum()) and not (h & cells).any()


def test_pack_roundtrip_odd_sizes():
    rng = np.random.default_rng(0)
    for dims in [(1, 1, 1), (31, 1, 1), (33, 2, 3), (97, 61, 45)]:
        c = rng.random(dims[::-1]) < 0.5
        w = solid_ref.pack(c)
        assert len(w) == (c.size + 31) // 32
        assert np.array_equal(solid_ref.unpack(w, dims), c)


def shell(n, lo, hi):
    c = np.zeros((n, n, n), bool)
    c[lo:hi + 1, lo:hi + 1, lo:hi + 1] = True
    c[lo + 1:hi, lo + 1:hi, lo + 1:hi] = False
    return c


def test_shell_is_filled():
    c = shell(9, 1, 7)
    s, h, n = fill_cells(c)
    assert n == 5 ** 3 and h[2:7, 2:7, 2:7].all() and h.sum() == n


def test_shell_with_one_cell_hole_leaks():
    c = shell(9, 1, 7)
    c[4, 4, 7] = False
    assert fill_cells(c)[2] == 0


def test_diagonal_gap_does_not_leak():
    """6-connectivity: a wall whose cells only touch along an edge still closes (an edge-diagonal step is not a path)."""
    c = shell(9, 1, 7)
    c[4, 4, 7] = False       # hole in the +x wall ...
    c[4, 4, 8] = True        # ... capped from outside, a step away: still closed
    c[4, 3, 8] = c[4, 5, 8] = c[3, 4, 8] = c[5, 4, 8] = False
    assert fill_cells(c)[2] == 5 ** 3 + 1


def test_nested_shells_fill_completely():
    c = shell(15, 1, 13) | shell(15, 5, 9)
    s, h, n = fill_cells(c)
    assert s[1:14, 1:14, 1:14].all() and n == 11 ** 3 - (5 ** 3 - 3 ** 3)


def test_torus_hole_stays_empty():
    n = 40
    z, y, x = np.mgrid[0:n, 0:n, 0:n] + 0.5
    r = np.hypot(x - n / 2, z - n / 2)
    d = np.hypot(r - 12, y - n / 2)
    c = (d <= 6) & (d >= 4.5)
    s, h, cnt = fill_cells(c)
    assert cnt > 0 and not s[n // 2, :, n // 2].any()        # the axis through the hole
    assert s[n // 2, n // 2, n // 2 + 12] and h[n // 2, n // 2, n // 2 + 12]  # the middle of the tube


@pytest.mark.parametrize("dims", [(1, 9, 9), (2, 9, 9), (9, 2, 9), (9, 9, 1), (1, 1, 1), (2, 2, 2)])
def test_thin_axes_have_no_interior(dims):
    X, Y, Z = dims
    c = np.zeros((Z, Y, X), bool)
    c[:, ::2, :] = True
    c[::2, :, :] = True
    assert fill_cells(c)[2] == 0


def test_rows_not_word_aligned():
    """X % 32 != 0: rows straddle words; the interior of a shell at the end of one row and the start of the next is kept apart."""
    c = np.zeros((7, 5, 37), bool)
    c[1:6, 1:4, 30:35] = True
    c[2:5, 2, 31:34] = False
    s, h, n = fill_cells(c)
    assert n == 9 and h[2:5, 2, 31:34].all()


def test_spiral_maze():
    cells = vx_scenes.spiral_maze(48)
    s, h, n = fill_cells(cells)
    assert n > 0 and h[24, 24, 24]
    open_core = vx_scenes.spiral_maze(48, closed_core=False)
    assert fill_cells(open_core)[2] == 0


def test_closed_scenes_are_closed_meshes():
    """every edge of the torus and of the nested shells is shared by exactly two triangles; the holed boxes have boundary edges"""
    def open_edges(t):
        e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        _, cnt = np.unique(e, axis=0, return_counts=True)
        return int((cnt != 2).sum())
    assert open_edges(vx_scenes.torus()[1]) == 0
    assert open_edges(vx_scenes.nested_shells()[1]) == 0
    assert open_edges(vx_scenes.holed_box(0.6)[1]) > 0


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--gpus", "2", "--logical"], ["--bench", "2"]])
def test_cli_solid_refusals(built, tmp_path, extra):
    obj = tmp_path / "c.obj"
    v, t = vx_scenes.cube()
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--solid"] + extra)
    assert r.returncode == 2 and "--solid fills the interior of one grid on one device" in r.stdout, r.stdout


def test_python_constant(vx):
    assert vx.VOXELIZE_SOLID == 4 and "vx_grid_fill_interior" in vx.SYMBOLS and "vx_grid_interior" in vx.SYMBOLS
