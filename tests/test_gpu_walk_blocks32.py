"""GPU tests of the traversal structure's block level at 32 cells: a block slab of k_walk and k_multihit is four brick slabs, the level-2
mip holds one bit per 4 x 4 x 4 bricks.  The cell planes w = 32, 96, 160 (and every other odd multiple of 32) are block boundaries now
and were not while a block was 64 cells; everything here happens at or across such a plane.

Grids built by hand, the reference is the oracle's brute force over the boxes of the occupied cells, t and prim are compared bit for bit
through the three first-hit query forms under VOXHIP_TRACE_LDS in {unset, 0} x VOXHIP_TRACE_DONATE in {unset, 0}, and trace_multi against
tests/multihit_ref.py (tests/walk_cases.py: check).  Constructions are written in the walk's permuted coordinates (u, v, w), w the rays'
major axis, per travel direction, and generated for the three major axes; each asserts on the CPU that it is what it claims to be."""
import functools

import numpy as np
import pytest

import oracle
import walk_cases as wc

pytestmark = pytest.mark.gpu

F = np.float32
ORIENTATIONS = wc.ORIENTATIONS
BOUNDARIES = (32, 96, 160)
CORRIDORS = [(16, 16, n) for n in (31, 32, 33, 40, 96, 160)]
WIDE = (8, 8, 70000)
D = (0.03, 0.02)   # the rays' slopes along u and v


# ---- 1. occupied cells on both sides of the new block boundaries ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straddle_scene(p, s, dims, boundaries=BOUNDARIES):
    """For every boundary B inside the grid: the last cell in front of it and the first cell behind it (in index order), at different
    (u, v), each with a bundle of rays through it alone, and one ray through both columns' gap that hits nothing."""
    sc = wc.scene(p, s, dims)
    nu, nv, nw = dims
    o, d, want = [], [], []
    for n, B in enumerate(boundaries):
        assert B % 32 == 0 and B % 64 == 32
        for cw, (cu, cv) in ((B - 1, (2, 5)), (B, (5, 2))):
            if not 0 <= cw < nw:
                continue
            cell = (cu + (n % 2), cv, cw)
            lin = sc.add(*cell)
            oo, dd = wc.ef.bundle(np.array(cell) + 0.5, (D[0], D[1], float(s)), 12.0, n=4, seed=cw)
            o.append(oo), d.append(dd), want.extend([lin] * 4)
    last = (8 % nu, 8 % nv, nw - 1)                                             # and the grid's last cell slab, whatever its length
    lin = sc.add(*last)
    oo, dd = wc.ef.bundle(np.array(last) + 0.5, (D[0], D[1], float(s)), 12.0, n=4, seed=nw)
    o.append(oo), d.append(dd), want.extend([lin] * 4)
    oo, dd = wc.through((0, 0, nw // 2), (0.0001, 0.0001, float(s)), 12.0)     # along the empty corner column
    o.append(oo[None]), d.append(dd[None]), want.append(-1)
    sc.finish(sc.make_rays(np.concatenate(o), np.concatenate(d)))
    assert np.array_equal(sc.ref_cell, np.array(want)), (sc.ref_cell, want)      # every bundle hits its own cell, first
    return sc


@pytest.mark.parametrize("dims", CORRIDORS, ids=lambda d: "w%d" % d[2])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_cells_on_both_sides_of_block_boundaries(gpu, p, s, dims):
    wc.check(gpu, straddle_scene(p, s, dims), shadow=True, big=dims[2] == 160)   # (big: the large-batch kernel walks the same blocks)


@pytest.mark.parametrize("s", [1, -1])
def test_cells_on_both_sides_of_block_boundaries_wide(gpu, s):
    """cell coordinates beyond 16 bits: the WIDE variant (the long axis is x, the only axis the ABI lets be that long with a small grid)"""
    wc.check(gpu, straddle_scene(0, s, WIDE, BOUNDARIES + (65568,)), shadow=True)


# ---- 2. rays that start inside, at the boundary ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inside_scene(p, s):
    """Origins inside a 16 x 16 x 96 corridor at w = 31.5, 32.0 (on the plane), 32.5 and 33.5; an occupied cell three cells ahead of every
    origin on its ray, and one two cells BEHIND it that the ray must not report."""
    sc = wc.scene(p, s, (16, 16, 96))
    o, d, want = [], [], []
    for n, w0 in enumerate((31.5, 32.0, 32.5, 33.5)):
        cu, cv = 3 + 3 * n, 4
        dd = np.array([D[0], D[1], float(s)])
        oo = np.array([cu + 0.5, cv + 0.5, w0])
        ahead = np.floor(oo + 3.0 * dd).astype(int)
        behind = np.floor(oo - 2.0 * dd).astype(int)
        assert ahead[2] != behind[2] and abs(ahead[2] - np.floor(w0)) <= 3
        want.append(sc.add(*ahead))
        sc.add(*behind)
        o.append(oo), d.append(dd)
    sc.finish(sc.make_rays(np.array(o), np.array(d)))
    assert np.array_equal(sc.ref_cell, np.array(want)) and len(sc.order) == 8
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_rays_that_start_at_a_block_boundary(gpu, p, s):
    wc.check(gpu, inside_scene(p, s), shadow=True)


# ---- 3. intervals that end one cell before and one cell after a boundary --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tmax_scene(p, s, B):
    """One occupied cell, the first of the block behind boundary B in travel order; rays straight along w from 12.5 cells in front of
    the plane (|d_w| = 1: t is the distance along w).  tmax_per_ray ends one cell before the plane (miss) and one cell after it (hit)."""
    sc = wc.scene(p, s, (16, 16, 192))
    cw = B if s > 0 else B - 1
    H = sc.add(6, 7, cw)
    o = np.array([[6.5, 7.5, B - s * 12.5]] * 2)
    d = np.array([[0.0005, 0.0003, float(s)]] * 2)
    sc.finish(sc.make_rays(o, d))
    assert np.all(sc.ref_cell == H) and np.all(np.abs(sc.ref_t - 12.5) < 1e-3)
    return sc, np.array([11.5, 13.5], F)


@pytest.mark.parametrize("B", BOUNDARIES)
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_tmax_one_cell_before_and_after_a_boundary(gpu, p, s, B):
    sc, tpr = tmax_scene(p, s, B)
    rt, rp = wc.rx.grid_closest_per_ray(wc.mr.hit_times(sc.oa, sc.rays), 0.001, tpr)
    assert rt[0] < 0 and rt[1] > 0 and rp[1] == 0                               # the short interval ends in front of the cell
    wc.check(gpu, sc, shadow=True, tmax_per_ray=tpr)


# ---- 4. donation cuts inside odd-numbered blocks --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_corridor_scene(p, s):
    """8 x 8 x 1024, occupied only in the last cell slab in travel order; 64 rays, one wave: every fourth points away from the grid and
    retires at refill, so 48 lanes are busy -- the donation threshold -- and the queue is dry from the start.  The rays start inside,
    `a` cells from the near end: k_walk cuts a ray's interval at its middle and starts the far piece one cell in front of the cut, so
    the first cut starts a piece in 32-cell block 17 (travelling up, a = 80.5, w about 552) or 13 (down, a = 160.5, w about 432)."""
    n, L = 64, 1024
    sc = wc.scene(p, s, (8, 8, L))
    wall = L - 1 if s > 0 else 0
    for cu in range(8):
        for cv in range(8):
            sc.add(cu, cv, wall)
    a = 80.5 if s > 0 else 160.5
    w0 = a if s > 0 else L - a
    cut = 0.5 * (a + L) if s > 0 else L - 0.5 * (a + L)                        # w of the first cut
    assert all(((int(cut) + e) >> 5) % 2 == 1 for e in (-2, -1, 0, 1, 2))     # an odd block, whichever way the slack cell falls
    rng = np.random.default_rng(7)
    o = np.concatenate([rng.uniform(1.0, 7.0, size=(n, 2)), np.full((n, 1), w0)], axis=1)
    tgt = np.concatenate([rng.uniform(1.0, 7.0, size=(n, 2)), np.full((n, 1), wall + 0.5)], axis=1)
    d = tgt - o
    away = np.arange(n) % 4 == 0
    d[away] = (0.01, 0.01, -float(s))
    o[away, 2] = -5.0 if s > 0 else L + 5.0
    sc.finish(sc.make_rays(o, d), tmax=20000.0)
    assert np.all(sc.ref_t[away] < 0) and np.all(sc.ref_t[~away] > 0)
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_split_rays_cut_inside_odd_blocks(gpu, p, s):
    wc.check(gpu, long_corridor_scene(p, s))


# ---- 5. ragged grids ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_scene(p, s, dims):
    """no dimension a multiple of the block (70 x 9 x 7: nor of the brick), the long axis along w; one cell in six occupied; rays from
    in front of the near end and from inside, mostly along w"""
    sc = wc.scene(p, s, dims)
    nu, nv, nw = dims
    rng = np.random.default_rng(nw)
    occ = rng.random((nw, nv, nu)) < 1.0 / 6.0
    for cw, cv, cu in np.argwhere(occ):
        sc.add(cu, cv, cw)
    n = 192
    o = np.stack([rng.uniform(0, nu, n), rng.uniform(0, nv, n), rng.uniform(-3.0, nw + 3.0, n)], axis=1)
    d = np.stack([rng.uniform(-0.12, 0.12, n), rng.uniform(-0.12, 0.12, n), np.full(n, float(s))], axis=1)
    sc.finish(sc.make_rays(o, d))
    cells = sc.ref_cell[sc.ref_cell >= 0]
    X, Y, Z = sc.dim
    xyz = np.stack([cells % X, (cells // X) % Y, cells // (X * Y)], axis=1)
    w = xyz[:, p]
    assert (sc.ref_t < 0).any() and (w < 32).any() and ((w >= 32) & (w < 64)).any() and (w >= 64).any()   # first hits in every block
    return sc


@pytest.mark.parametrize("dims", [(9, 7, 70), (8, 5, 96)], ids=["70x9x7", "96x8x5"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_ragged_grids(gpu, p, s, dims):
    wc.check(gpu, ragged_scene(p, s, dims), shadow=True, big=True)


# ---- 6. a voxelized mesh --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_reference():
    import vx_scenes
    v, t = vx_scenes.scene("blob70k")
    vs = F((v.max(0) - v.min(0)).max() / 96.0 * 1.0001)
    ow, _, gi = oracle.build_bool(v, t, vs)
    oa = oracle.bool_aabbs(ow, gi, vs)
    rays = vx_scenes.random_rays(20000, gi["bmin"], gi["bmax"], seed=2)
    rt, rp = oracle.trace_brute(oa, rays, threads=8)
    assert max(gi["dim"]) in (96, 97) and min(gi["dim"]) > 64 and (rt > 0).sum() > 5000 and (rt < 0).sum() > 1000
    return v, t, vs, ow, gi, oa, rays, rt, rp


def test_blob_at_96_cubed(gpu):
    """three block slabs per axis, rays of every major axis and direction"""
    v, t, vs, ow, gi, oa, rays, rt, rp = blob_reference()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), vs, gpu.GRID_BOOL)
    try:
        assert g.describe()["dim"] == gi["dim"] and np.array_equal(g.bitmask(), ow)
        for lds, don in wc.ENVS:
            with wc.ef.env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=don):
                tt, pp, nh = g.trace(rays)
                assert wc.same_bits(tt, rt) and np.array_equal(pp, rp) and nh == int((rt > 0).sum()), (lds, don)
        sub = rays[:256]
        mt, mp, mc = wc.mr.multi(oa, sub, wc.K_MULTI)
        got = g.trace_multi(sub, max_hits=wc.K_MULTI)
        assert wc.same_bits(got["t"], mt) and np.array_equal(got["prim"], mp) and np.array_equal(got["count"], mc)
    finally:
        g.free()
