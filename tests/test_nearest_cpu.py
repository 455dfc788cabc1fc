"""CPU tests of the feature transform: the three restatements (tests/nearest_ref.py: the definition, the separable numpy form, the C
helper) against each other, the squared distance of the nearest cell against the distance fields' restatement, the sentinels, the
cross-compiled library's exports and NULL-grid check, and the CLI's refusals of --nearest (all of them run before any device is touched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distance_ref
import nearest_ref as nr
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")

# every size from 1 to 9 on every axis
DIMS = [(a, (a * 4) % 9 + 1, (a * 7) % 9 + 1) for a in range(1, 10)]
DIMS += [(z, x, y) for (x, y, z) in DIMS] + [(y, z, x) for (x, y, z) in DIMS]


@pytest.mark.parametrize("dims", DIMS)
def test_the_three_forms_agree(dims):
    rng = np.random.default_rng(sum(dims) * 31 + dims[0])
    X, Y, Z = dims
    for p in (0.0, 0.08, 0.3, 0.5, 1.0):
        m = rng.random((Z, Y, X)) < p
        for target in (m, ~m):
            want = nr.brute(target)
            assert np.array_equal(nr.nearest(target), want), (dims, p)
            assert np.array_equal(nr.nearest_c(target), want), (dims, p)
            assert np.array_equal(nr.dist_sq_of(want), distance_ref.brute_sq(target)), (dims, p)


def tie_masks():
    """masks whose nearest targets tie: the distance is the same whichever wins, the index is not"""
    out = []
    m = np.zeros((9, 9, 9), bool)
    m[::8, ::8, ::8] = True  # the 8 corners: the centre is 8 ways tied
    out.append(("corners", m))
    m = np.zeros((14, 15, 16), bool)
    m[::2, ::2, ::2] = True
    out.append(("lattice", m))
    m = np.zeros((13, 12, 12), bool)
    m[2] = True
    m[10] = True
    out.append(("planes", m))
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = 9
        m = np.zeros(shape, bool).reshape(-1)
        m[3] = m[5] = True
        out.append(("pair%d" % axis, m.reshape(shape)))
    return out


@pytest.mark.parametrize("name,m", tie_masks(), ids=[n for n, _ in tie_masks()])
def test_ties_go_to_the_smallest_index(name, m):
    for target in (m, ~m):
        want = nr.brute(target)
        assert np.array_equal(nr.nearest(target), want)
        assert np.array_equal(nr.nearest_c(target), want)
    if name == "corners":
        assert nr.brute(m)[4, 4, 4] == 0
    if name.startswith("pair"):
        got = nr.brute(m).reshape(-1)
        step = (m.shape[2] * m.shape[1] if m.shape[0] == 9 else m.shape[2] if m.shape[1] == 9 else 1)
        assert got[4] == 3 * step and got[3] == 3 * step and got[5] == 5 * step and got[8] == 5 * step


def test_tied_cells_are_common_in_the_random_grids():
    """the agreement above is about ties too: a good share of the cells of a random grid has more than one nearest target"""
    rng = np.random.default_rng(5)
    tied = cells = 0
    for _ in range(20):
        m = rng.random((6, 6, 6)) < 0.2
        idx = np.flatnonzero(m.reshape(-1))
        if not idx.size:
            continue
        zz, yy, xx = np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")
        c = np.stack([zz.reshape(-1), yy.reshape(-1), xx.reshape(-1)], 1)
        d = ((c[:, None, :] - c[None, idx, :]) ** 2).sum(-1)
        tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
        cells += d.shape[0]
    assert tied * 10 > cells


def test_squared_distance_of_the_nearest_cell_is_the_distance_field():
    rng = np.random.default_rng(9)
    for shape, p in (((13, 17, 19), 0.01), ((8, 40, 33), 0.3), ((31, 5, 64), 0.002)):
        m = rng.random(shape) < p
        m[0, 0, 0] = True
        m[-1, -1, -1] = False
        for target in (m, ~m):
            n = nr.nearest(target)
            assert np.array_equal(nr.dist_sq_of(n), distance_ref.edt_sq(target))
            assert target.reshape(-1)[n.reshape(-1)].all()  # every N is a target cell
            own = np.arange(n.size, dtype=np.uint32).reshape(n.shape)
            assert np.array_equal(n[target], own[target])  # N(c) = i(c) on T


def test_c_helper_matches_numpy_on_larger_masks():
    rng = np.random.default_rng(3)
    for shape, p in (((20, 30, 70), 0.001), ((50, 3, 41), 0.2), ((1, 1, 3000), 0.001), ((200, 2, 2), 0.01), ((2, 300, 3), 0.01)):
        m = rng.random(shape) < p
        for target in (m, ~m):
            assert np.array_equal(nr.nearest_c(target), nr.nearest(target)), shape


def test_empty_and_full_masks_give_the_sentinel():
    m = np.zeros((3, 4, 5), bool)
    for f in (nr.brute, nr.nearest, nr.nearest_c):
        assert (f(m) == 0xFFFFFFFF).all()
        assert np.array_equal(f(~m).reshape(-1), np.arange(60, dtype=np.uint32))
    n = nr.nearest(m)
    assert (nr.dist_sq_of(n) == 0xFFFFFFFF).all()
    assert (nr.gather(n, np.arange(60), 7) == 7).all()
    assert np.array_equal(nr.gather(nr.nearest(~m), np.arange(60) * 3, 7).reshape(-1), np.arange(60, dtype=np.uint32) * 3)


def test_library_exports_the_nearest_entry_points(vx):
    L = ctypes.CDLL(vx.LIB_PATH)
    for n in ("vx_grid_nearest_device", "vx_grid_nearest", "vx_grid_nearest_gather_device", "vx_grid_nearest_gather"):
        assert hasattr(L, n) and n in vx.SYMBOLS, n
    for n in ("nearest", "nearest_device", "nearest_gather", "nearest_gather_device", "nearest_labels"):
        assert callable(getattr(vx.Grid, n)), n


def test_null_grid_is_invalid(vx):
    L = vx.lib()
    buf = np.zeros(8, np.uint32)
    val = np.ones(8, np.uint32)
    assert L.vx_grid_nearest(None, 0, buf.ctypes.data, 8) == 1
    assert L.vx_grid_nearest_device(None, 0, buf.ctypes.data, 8) == 1
    assert L.vx_grid_nearest_gather(None, 0, val.ctypes.data, 8, 5, buf.ctypes.data, 8) == 1
    assert L.vx_grid_nearest_gather_device(None, 0, val.ctypes.data, 8, 5, buf.ctypes.data, 8) == 1
    assert (buf == 0).all()


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--bench", "2"]])
def test_cli_nearest_refusals(built, tmp_path, extra):
    obj = tmp_path / "c.obj"
    v, t = vx_scenes.cube()
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--nearest", str(tmp_path / "n.bin")] + extra)
    assert r.returncode == 2 and "--nearest writes the nearest-cell field of one grid on one device" in r.stdout, r.stdout
    assert not (tmp_path / "n.bin").exists()


def test_cli_nearest_inside_needs_nearest(built, tmp_path):
    obj = tmp_path / "c.obj"
    v, t = vx_scenes.cube()
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--nearest-inside"])
    assert r.returncode == 2 and "--nearest" in r.stdout, r.stdout
