"""CPU tests of the connected-component restatement (tests/components_ref.py): hook-and-jump union-find against scipy.ndimage.label,
against the C helper, on hand-worked cases, and the statistics against brute force."""
import numpy as np
import pytest

import components_ref as cr

CONN = [6, 26]


def scipy_label(cells, connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    lab, k = nd.label(cells, structure=nd.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    return lab.astype(np.uint32), int(k)


@pytest.mark.parametrize("connectivity", CONN)
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 97), (13, 1, 7), (1, 29, 1), (33, 17, 9), (31, 23, 19)])
@pytest.mark.parametrize("density", [0.05, 0.10, 0.31, 0.5, 0.9])
def test_matches_scipy(connectivity, dims, density):
    X, Y, Z = dims
    cells = np.random.default_rng(X * 131 + Y * 17 + Z + int(density * 100) + connectivity).random((Z, Y, X)) < density
    want, kw = scipy_label(cells, connectivity)
    got, k = cr.label(cells, connectivity)
    assert k == kw and np.array_equal(got, want)
    gc, kc = cr.label_c(cells, connectivity)
    assert kc == kw and np.array_equal(gc, want)


@pytest.mark.parametrize("connectivity", CONN)
def test_c_helper_matches_numpy(connectivity):
    rng = np.random.default_rng(5)
    for dims, density in (((64, 48, 40), 0.31), ((70, 30, 50), 0.10), ((128, 8, 8), 0.6), ((3, 3, 2000), 0.7)):
        X, Y, Z = dims
        cells = rng.random((Z, Y, X)) < density
        a, ka = cr.label(cells, connectivity)
        b, kb = cr.label_c(cells, connectivity)
        assert ka == kb and np.array_equal(a, b)
        assert np.array_equal(cr.stats(a, ka), cr.stats(b, kb))


def test_checkerboard():
    Z = Y = X = 8
    z, y, x = np.indices((Z, Y, X))
    cells = (x + y + z) % 2 == 0
    lab6, k6 = cr.label(cells, 6)
    assert k6 == cells.size // 2 and np.array_equal(lab6[cells], np.arange(1, k6 + 1))
    lab26, k26 = cr.label(cells, 26)
    assert k26 == 1 and (lab26[cells] == 1).all() and (lab26[~cells] == 0).all()


@pytest.mark.parametrize("shift,k6", [((1, 1, 1), 2), ((0, 1, 1), 2), ((1, 0, 1), 2), ((0, 0, 1), 1)])
def test_corner_and_edge_contacts(shift, k6):
    cells = np.zeros((4, 4, 4), bool)
    cells[1, 1, 1] = True
    dz, dy, dx = shift
    cells[1 + dz, 1 + dy, 1 + dx] = True
    assert cr.label(cells, 6)[1] == k6
    assert cr.label(cells, 26)[1] == 1


def test_nested_shells():
    n = 11
    cells = np.zeros((n, n, n), bool)
    cells[:] = True
    cells[1:-1, 1:-1, 1:-1] = False      # outer shell
    cells[3:-3, 3:-3, 3:-3] = True
    cells[4:-4, 4:-4, 4:-4] = False      # inner shell
    cells[5, 5, 5] = True                # a core cell
    for c in CONN:
        lab, k = cr.label(cells, c)
        assert k == 3
        assert lab[0, 0, 0] == 1 and lab[3, 3, 3] == 2 and lab[5, 5, 5] == 3


def test_numbering_by_smallest_cell():
    # A is found first along its bottom row, but its smallest cell is the top of its column (index 5): labels follow smallest cells
    cells = np.zeros((1, 4, 6), bool)
    cells[0, 3, :] = True     # A: the bottom row ...
    cells[0, :, 5] = True     # ... and a column up to (x=5, y=0)
    cells[0, 0, 1] = True     # B: index 1
    cells[0, 1, 2] = True     # C: index 8, diagonal to B
    lab, k = cr.label(cells, 6)
    assert k == 3
    assert lab[0, 0, 1] == 1 and lab[0, 0, 5] == 2 and lab[0, 3, 0] == 2 and lab[0, 1, 2] == 3
    lab26, k26 = cr.label(cells, 26)
    assert k26 == 2 and lab26[0, 0, 1] == lab26[0, 1, 2] == 1 and lab26[0, 3, 0] == 2


@pytest.mark.parametrize("connectivity", CONN)
def test_stats_against_brute_force(connectivity):
    cells = np.random.default_rng(9).random((9, 14, 23)) < 0.3
    lab, k = cr.label(cells, connectivity)
    s = cr.stats(lab, k)
    assert s.dtype.itemsize == 32 and len(s) == k
    assert s.tobytes() == cr.brute_stats(lab, k).tobytes()
    assert int(s["cells"].sum()) == int(cells.sum())


def test_empty_and_full():
    for c in CONN:
        lab, k = cr.label(np.zeros((3, 4, 5), bool), c)
        assert k == 0 and not lab.any() and len(cr.stats(lab, k)) == 0
        lab, k = cr.label(np.ones((3, 4, 5), bool), c)
        assert k == 1 and (lab == 1).all()
        s = cr.stats(lab, k)
        assert s[0]["cells"] == 60 and tuple(s[0]["min"]) == (0, 0, 0) and tuple(s[0]["max"]) == (4, 3, 2)


def test_library_exports_and_refuses_null_grid(vx):
    import ctypes
    L = ctypes.CDLL(vx.LIB_PATH)
    for name in ("vx_grid_components_device", "vx_grid_components", "vx_grid_component_stats"):
        assert hasattr(L, name)
    assert vx.COMPONENT.itemsize == 32 and (vx.CONNECT_6, vx.CONNECT_26) == (6, 26)
    k = ctypes.c_uint64(7)
    assert vx.lib().vx_grid_components(None, 6, None, 0, ctypes.byref(k)) == 1 and k.value == 7  # VX_ERR_INVALID_ARG, nothing written
    assert vx.lib().vx_grid_component_stats(None, 26, None, 0, ctypes.byref(k)) == 1 and k.value == 7
    assert vx.lib().vx_grid_components_device(None, 6, None, 0, None) == 1
