"""The surface-nets restatement (tests/nets_ref.py) against its own per-vertex loop, against surface_ref's topology, and against the
properties the contract states: bounds, the blocky mesh at zero offsets, pinned small cases and the roundness of a voxel ball.  No GPU."""
import numpy as np
import pytest

import nets_ref as nr
import surface_ref as sr

F = np.float32
ORG = (0.25, -1.0, 3.0)
VS = F(0.37)


def random_cells(dims, density):
    X, Y, Z = dims
    return np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density


@pytest.mark.parametrize("dims", [(5, 3, 2), (9, 8, 7), (12, 12, 12)])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("params", [(0, 0.5, -0.53), (3, 0.5, -0.53), (2, 1.0, 0.0)])
def test_vectorised_equals_brute(dims, density, params):
    cells = random_cells(dims, density)
    it, lam, mu = params
    P, N, u0, u, n, m, used = nr.brute(cells, ORG, VS, it, lam, mu)
    v_used, ijk, cfg, nbr, v_u0, v_u = nr.offsets(cells, it, lam, mu)
    assert np.array_equal(used, v_used)
    assert u0.tobytes() == v_u0.tobytes() and u.tobytes() == v_u.tobytes()
    verts, tris, normals = nr.surface_smooth(cells, ORG, VS, it, lam, mu, with_normals=True)
    assert verts.tobytes() == P.tobytes()
    assert normals.tobytes() == N.tobytes()
    # vertex set and triangles are the blocky mesh's
    b_used, b_tris, _, _ = sr.surface_lattice(cells)
    assert np.array_equal(b_used, used) and np.array_equal(sr.mixed_corners(cells), used)
    assert tris.tobytes() == b_tris.tobytes()
    # bounds
    assert np.array_equal(n, nr.N_TAB[cfg]) and np.array_equal(m, (nbr >= 0).sum(axis=1))
    if len(used):
        assert n.min() >= 3 and n.max() <= 12 and m.min() >= 3
        assert np.abs(u0).max() <= F(1.0) / F(3.0) and np.abs(u).max() <= 0.5


def test_every_configuration_has_three_crossings_and_neighbours():
    mixed = np.arange(1, 255)
    assert nr.N_TAB[mixed].min() >= 3 and nr.N_TAB[mixed].max() <= 12
    assert nr.NB_TAB[mixed].sum(axis=1).min() >= 3
    assert (np.abs(nr.T_TAB[mixed]) * 3 <= 2 * nr.N_TAB[mixed][:, None]).all()   # |u0| <= 1/3


def test_zero_offsets_give_the_blocky_positions():
    cells = np.ones((5, 3, 4), bool)   # X, Y, Z = 4, 3, 5
    used, ijk, cfg, nbr, u0, u = nr.offsets(cells, 0)
    X, Y, Z = 4, 3, 5
    inner = np.zeros(len(used), bool)
    for a, n in enumerate((X, Y, Z)):
        o = [b for b in range(3) if b != a]
        on = (ijk[:, a] == 0) | (ijk[:, a] == n)
        inside = np.ones(len(used), bool)
        for b in o:
            inside &= (ijk[:, b] > 0) & (ijk[:, b] < (X, Y, Z)[b])
        inner |= on & inside
    assert inner.sum() == 2 * (2 * 3 + 2 * 4 + 3 * 4)   # (Y-1)(X-1) etc. per pair of faces
    assert (u0[inner] == 0).all() and not np.signbit(u0[inner]).any()
    zero = np.zeros_like(u0)
    assert nr.positions(ijk, zero, ORG, VS).tobytes() == sr.positions(ijk, ORG, VS).tobytes()
    v0 = nr.surface_smooth(cells, ORG, VS, 0)[0]
    assert v0[inner].tobytes() == sr.surface(cells, ORG, VS)[0][inner].tobytes()


def _cells(dim, occupied):
    c = np.zeros(dim[::-1], bool)
    for x, y, z in occupied:
        c[z, y, x] = True
    return c


def test_pinned_small_cases():
    one = _cells((1, 1, 1), [(0, 0, 0)])
    v, t, nrm = nr.surface_smooth(one, (0, 0, 0), F(1), 0, with_normals=True)
    assert v.shape == (8, 3) and t.shape == (12, 3)
    # each corner moves a third of a cell towards the centre along every axis: n = 3, T = +-2
    want = np.array([[(F(b) + F(0.5) + (F(2 - 4 * b) / F(6))) * F(1) - F(0.5) for b in ((c & 1), (c >> 1) & 1, c >> 2)] for c in range(8)], np.float32)
    assert v.tobytes() == want.tobytes()
    d = v - v.mean(axis=0)
    assert ((nrm * d).sum(axis=1) > 0).all()
    edge = _cells((2, 2, 1), [(0, 0, 0), (1, 1, 0)])
    v, t = nr.surface_smooth(edge, (0, 0, 0), F(1), 4)
    assert (len(v), len(t)) == (14, 24)
    corner = _cells((2, 2, 2), [(0, 0, 0), (1, 1, 1)])
    v, t = nr.surface_smooth(corner, (0, 0, 0), F(1), 4)
    assert (len(v), len(t)) == (15, 24)
    for c in (edge, corner):
        _, _, cfg, nbr, _, _ = nr.offsets(c, 0)
        assert nr.N_TAB[cfg].min() >= 3 and (nbr >= 0).sum(axis=1).min() >= 3


def test_parameter_ranges():
    assert nr.check_params(0, 0.0, 0.0) and nr.check_params(1024, 1.0, -1.0)
    for bad in ((1025, 0.5, 0.0), (1, np.nan, 0.0), (1, 1.5, 0.0), (1, 0.5, 0.1), (1, 0.5, -np.inf), (1, -0.1, 0.0), (1, 0.5, -1.5)):
        assert not nr.check_params(*bad)


def _ball(n, R):
    c = (np.arange(n) + 0.5) - n / 2.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return x * x + y * y + z * z <= R * R


def _radii(v, n):
    return np.linalg.norm(v.astype(np.float64) - n / 2.0, axis=1)


def test_ball_gets_rounder():
    n, R = 16, 6.0
    cells = _ball(n, R)
    org, vs = (0.0, 0.0, 0.0), F(1)
    blocky = _radii(sr.surface(cells, org, vs)[0], n)
    r0 = _radii(nr.surface_smooth(cells, org, vs, 0)[0], n)
    r2 = _radii(nr.surface_smooth(cells, org, vs, 2, 1.0, 0.0)[0], n)
    v16, _, nrm = nr.surface_smooth(cells, org, vs, 16, 0.5, -0.53, with_normals=True)
    r16 = _radii(v16, n)
    assert len(r0) == 674
    assert r0.std() < 0.5 * blocky.std()
    assert r2.std() < r0.std()
    assert abs(r16.mean() - r0.mean()) < 0.1
    radial = v16.astype(np.float64) - n / 2.0
    assert ((nrm * radial).sum(axis=1) > 0).all()
