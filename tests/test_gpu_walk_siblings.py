"""GPU tests of how k_walk goes through the occupied bricks of one brick slab's rectangle -- the sibling bricks: which of them it looks at
first, and which it may leave out once a hit is known (a brick the ray cannot enter before the best hit).  Every case is a situation in
which visiting the siblings in travel order, or dropping one by the time the ray crosses its entry plane, could lose the closest hit or
the lower voxel index of a tie.

64^3 grids, voxel size 1 and origin 0 unless a case needs rounded planes and says so.  Grids built by hand, the reference is the oracle's
brute force, t and prim are compared bit for bit through the three first-hit query forms under VOXHIP_TRACE_LDS in {unset, 0} x
VOXHIP_TRACE_DONATE in {unset, 0}, with any_hit and a per-ray tmax on top -- and, under the same four switch pairs, again as a batch of
1 064 960 rays, the size from which launch_walk takes the kernel that orders and prunes the siblings: smaller batches run the kernel
without that code (tests/walk_cases.py: check, big).  Constructions are written in the
walk's permuted coordinates (u, v, w) per travel direction and generated for the three major axes; each asserts on the CPU what it claims."""
import functools
import types

import numpy as np
import pytest

import walk_cases as wc

pytestmark = pytest.mark.gpu

F = np.float32
ORIENTATIONS = wc.ORIENTATIONS
G64 = (64, 64, 64)
DOWN = [(-1, 1), (1, -1), (-1, -1)]                           # (travel along u, along v): down u, down v, down both
SIGNS = [(1, 1)] + DOWN


def brick(c):
    return (int(c[0]) >> 3, int(c[1]) >> 3)


def line(P, d):
    """w -> the ray's point at that w, for a ray through P with direction d (d_w = +-1)"""
    P, d = np.array(P, np.float64), np.array(d, np.float64)
    return lambda w: P + (w - P[2]) / d[2] * d


def ray_along(P, d, back=18.0, n=6, seed=0):
    return wc.ef.bundle(P, d, back, n=n, seed=seed)


# ---- 1. the hit is in the first brick, the sibling has nothing inside the rectangle ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def empty_sibling_scene(p, s):
    """Brick slab 3 (w in [24, 32)); the ray crosses u = 32 inside it, so the slab's rectangle spans two bricks.  The hit cell is in the
    brick the ray is in first; the other brick is occupied (its level-1 bit is set) only at its far corner, which the ray never touches."""
    sc = wc.scene(p, s, G64)
    d = (0.2, 0.01, float(s))
    at = line((32.0, 19.5, 28.0), d)
    w_hit = 25 if s > 0 else 30                                 # an early cell slab of the brick slab in travel order
    hit = np.floor(at(w_hit + 0.5)).astype(int)
    other = (39, 23, 24 if s > 0 else 31) if brick(hit)[0] == 3 else (24, 16, 24 if s > 0 else 31)
    H, Ot = sc.add(*hit), sc.add(*other)
    assert brick(hit) != brick(other) and brick(hit)[1] == brick(other)[1] and abs(brick(hit)[0] - brick(other)[0]) == 1
    o, dd = ray_along((32.0, 19.5, 28.0), d)
    sc.finish(sc.make_rays(o, dd))
    assert np.all(sc.ref_cell == H) and np.all(sc.alone(Ot) < 0)
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_hit_in_first_brick_sibling_empty_in_rectangle(gpu, p, s):
    wc.check(gpu, empty_sibling_scene(p, s), shadow=True, big=True)


# ---- 2. the closer cell is in the brick with the higher index -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def higher_brick_first_scene(p, s, su, sv):
    """The ray travels down u, down v or down both and crosses u = 32 and / or v = 16 in the middle of brick slab 3: the brick it is in
    first has the HIGHER index along every axis it travels down -- index order would fetch it last.  The near cell is there, a farther one
    in the brick the ray ends in."""
    sc = wc.scene(p, s, G64)
    d = (0.5 * su if su < 0 else 0.01, 0.5 * sv if sv < 0 else 0.01, float(s))
    P = (32.0 if su < 0 else 19.5, 16.0 if sv < 0 else 19.5, 28.0)
    at = line(P, d)
    w_near, w_far = (25, 30) if s > 0 else (30, 25)
    near, far = np.floor(at(w_near + 0.5)).astype(int), np.floor(at(w_far + 0.5)).astype(int)
    N, Fr = sc.add(*near), sc.add(*far)
    bn, bf = brick(near), brick(far)
    assert bn != bf and bn[0] >= bf[0] and bn[1] >= bf[1] and (near[2] >> 3) == (far[2] >> 3) == 3
    assert (bn[0] > bf[0]) == (su < 0) and (bn[1] > bf[1]) == (sv < 0)
    o, dd = ray_along(P, d)
    sc.finish(sc.make_rays(o, dd))
    assert sc.ref_cell[0] == N and sc.alone(Fr)[0] > sc.ref_t[0] > 0             # both are hit, the one in the higher brick first
    return sc


@pytest.mark.parametrize("su,sv", DOWN, ids=["down-u", "down-v", "down-both"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_closer_cell_in_brick_of_higher_index(gpu, p, s, su, sv):
    sc = higher_brick_first_scene(p, s, su, sv)
    wc.check(gpu, sc, shadow=True, tmax_per_ray=wc.at_and_below(sc), big=True)   # (tmax at the hit / just short of it)


# ---- 3. an equal t in the sibling, with the lower voxel index -------------------------------------------------------------------------
TIE_B = 48   # a brick boundary along u at which, with voxel size 0.1 and origin 0.3, the rounded planes of the cells on its two sides overlap


@functools.lru_cache(maxsize=None)
def tie_scene(p, s, su):
    """Two cells side by side along u across the brick boundary u = TIE_B, in the same cell slab, entered through their common w plane:
    with voxel size 0.1 and origin 0.3 the upper u plane of cell TIE_B - 1 is one ulp above the lower u plane of cell TIE_B, and a ray
    that runs (all but) along that sliver -- |d_u| = 1e-20, u between the two planes -- is inside both boxes when it reaches the w plane:
    both report that plane's time, the same float.  The rectangle is two bricks wide by the tolerance alone.  su is the sign of d_u:
    travelling down u the brick of cell TIE_B comes first and the lower voxel index waits in the sibling."""
    sc = wc.scene(p, s, G64, vs=0.1, org=0.3)
    cv, k = 19, 27
    A, B = sc.add(TIE_B - 1, cv, k), sc.add(TIE_B, cv, k)
    sc.finish(np.ones((1, 6), F))                                               # (only the boxes are wanted)
    ia, ib = int(np.searchsorted(sc.order, A)), int(np.searchsorted(sc.order, B))
    pu, pv = (p + 1) % 3, (p + 2) % 3
    mxA, mnB = sc.oa["mx"][ia, pu], sc.oa["mn"][ib, pu]
    assert mxA > mnB and np.nextafter(mnB, F(np.inf)) == mxA                    # the one-ulp overlap
    vc = 0.5 * (float(sc.oa["mn"][ia, pv]) + float(sc.oa["mx"][ia, pv]))
    wlo, whi = float(sc.oa["mn"][ia, p]), float(sc.oa["mx"][ia, p])
    r = np.zeros((8, 6))
    for j in range(8):
        r[j, p] = (wlo - 1.5 - 0.125 * j) if s > 0 else (whi + 1.5 + 0.125 * j)
        r[j, pu] = float(mxA if su < 0 else mnB)                                # the plane that is NOT multiplied by zero distance
        r[j, pv] = vc
        r[j, 3 + p], r[j, 3 + pu], r[j, 3 + pv] = float(s), su * 1e-20, 1e-20
    rays = np.ascontiguousarray(r.astype(F))
    sc.finish(rays)
    ta, tb = sc.alone(A), sc.alone(B)
    assert np.all(ta > 0) and wc.same_bits(ta, tb) and wc.same_bits(sc.ref_t, ta)   # the exact tie, on every ray
    assert np.all(sc.ref_cell == min(A, B)) and A < B
    tol = wc.kernel_tol(sc)
    assert np.all(tol > float(np.spacing(mxA)))                                 # both cells are inside the rectangle, by tolerance only
    return sc


@pytest.mark.parametrize("su", [1, -1], ids=["up-u", "down-u"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_equal_t_in_sibling_with_lower_voxel_index(gpu, p, s, su):
    sc = tie_scene(p, s, su)
    wc.check(gpu, sc, shadow=True, tmax_per_ray=wc.at_and_below(sc), big=True)


# ---- 4. a sibling cell whose box starts within a few ulps of the entry plane ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grazing_entry_scene(p, s, su):
    """Voxel size 0.1, origin 0.3: cells TIE_B - 1 and TIE_B side by side along u in cell slab k, in two bricks, and the rays cross the
    brick boundary within a few ulps of the moment they cross into the slab -- through the edge the two boxes share, origins stepped by
    half ulps across it.  Whichever brick is looked at first, the other one's only cell starts at its entry plane, and the two boxes'
    times differ by a few ulps or not at all; the brute force says which wins."""
    sc = wc.scene(p, s, G64, vs=0.1, org=0.3)
    cv, k = 19, 27
    A, B = sc.add(TIE_B - 1, cv, k), sc.add(TIE_B, cv, k)
    sc.finish(np.ones((1, 6), F))
    ia = int(np.searchsorted(sc.order, A))
    pu, pv = (p + 1) % 3, (p + 2) % 3
    Pu = float(sc.oa["mx"][ia, pu])                                             # the shared u plane
    Pw = float(sc.oa["mn"][ia, p] if s > 0 else sc.oa["mx"][ia, p])             # the w plane the rays enter the slab through
    vc = 0.5 * (float(sc.oa["mn"][ia, pv]) + float(sc.oa["mx"][ia, pv]))
    ulp = float(np.spacing(F(Pu)))
    rows = []
    for T in (1.5, 1.25, 1.75):
        for j in range(-12, 13):
            r = np.zeros(6)
            r[p], r[pu], r[pv] = Pw - s * T, Pu - su * 0.5 * T + 0.5 * j * ulp, vc - 0.001 * T
            r[3 + p], r[3 + pu], r[3 + pv] = float(s), su * 0.5, 0.001
            rows.append(r)
    rays = np.ascontiguousarray(np.array(rows).astype(F))
    sc.finish(rays)
    ta, tb = sc.alone(A), sc.alone(B)
    both = (ta > 0) & (tb > 0)
    close = both & (np.abs(ta - tb) <= 8 * np.spacing(np.maximum(ta, tb)))
    one = (ta > 0) ^ (tb > 0)
    assert close.sum() >= 4 and one.sum() >= 4, (int(close.sum()), int(one.sum()))  # rays through both within ulps, and rays that miss one
    return sc


@pytest.mark.parametrize("su", [1, -1], ids=["up-u", "down-u"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_sibling_cell_starts_at_the_entry_plane(gpu, p, s, su):
    sc = grazing_entry_scene(p, s, su)
    wc.check(gpu, sc, shadow=True, tmax_per_ray=wc.at_and_below(sc), big=True)


# ---- 5. rays exactly on a brick edge --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def on_edge_scene(p, s, zu, zv):
    """Rays along w with d_u == 0 and / or d_v == 0 exactly (and its negative zero), ON the lattice plane u = 32 and / or v = 16 -- the
    brick edge -- and one ulp to either side of it: the rectangle is two bricks wide (four around the corner) by the tolerance alone.
    One occupied cell in every brick around the edge, next to it, in different cell slabs.  On the plane itself 0 * inf makes every
    neighbouring box a miss; an ulp beside it the ray runs through one column of cells."""
    sc = wc.scene(p, s, G64)
    us = (31, 32) if zu else (19,)
    vs_ = (15, 16) if zv else (19,)
    for n, (cu, cv) in enumerate([(a, b) for b in vs_ for a in us]):
        sc.add(cu, cv, 25 + n)
        sc.add(cu, cv, 30 - n)
    rows = []
    for zero in (0.0, -0.0):
        for eu in ((-1, 0, 1) if zu else (0,)):
            for ev in ((-1, 0, 1) if zv else (0,)):
                ou = float(np.nextafter(F(32.0), F(32.0 + eu))) if zu else 19.4
                ov = float(np.nextafter(F(16.0), F(16.0 + ev))) if zv else 19.6
                rows.append([ou, ov, 28.0 - s * 18.0, zero if zu else 0.013, zero if zv else -0.011, float(s)])
    r = np.array(rows)
    sc.finish(sc.make_rays(r[:, :3], r[:, 3:]))
    du, dv = sc.rays[:, 3 + (p + 1) % 3], sc.rays[:, 3 + (p + 2) % 3]
    assert (not zu or np.all(du == 0)) and (not zv or np.all(dv == 0)) and np.signbit(sc.rays[:, 3:]).any()
    on = np.array([(not zu or row[0] == 32.0) and (not zv or row[1] == 16.0) for row in rows])
    beside = np.array([(not zu or row[0] != 32.0) and (not zv or row[1] != 16.0) for row in rows])
    assert np.all(sc.ref_t[on] < 0) and np.all(sc.ref_t[beside] > 0) and on.sum() == 2 and beside.any()
    assert np.all(wc.kernel_tol(sc) > float(np.spacing(F(32.0))))               # an ulp is inside the tolerance: both bricks in the rectangle
    return sc


@pytest.mark.parametrize("zu,zv", [(True, False), (False, True), (True, True)], ids=["du0", "dv0", "both0"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_rays_on_a_brick_edge_with_zero_components(gpu, p, s, zu, zv):
    wc.check(gpu, on_edge_scene(p, s, zu, zv), shadow=True, big=True)


# ---- 6. all four bricks of a 2 x 2 occupied, the ray through three of them ------------------------------------------------------------
# which boundary the ray crosses first, and the brick of its path that holds the nearest hit: every brick of the path once, both orders of the
# crossings (three of the six pairs; tests/test_gpu_walk_early_finish.py runs all six for travel down u and v -- with four travel sign
# pairs, six orientations and the large batch under four switch pairs, six would be 144 cases of a second each)
QUAD = [("v", 0), ("u", 1), ("v", 2)]


@functools.lru_cache(maxsize=None)
def quad_scene(p, s, su, sv, first, target):
    """The 2 x 2 form for every pair of travel signs along u and v: the ray crosses u = 32 and v = 16 inside brick slab 3, one at w = 26.6
    and the other at w = 28 (mirrored when travelling down w), so its path runs through three of the four bricks around the corner.
    Brick `target` of the path holds the nearest hit, every later brick of the path a farther one, every other brick an occupied cell
    at the corner, beside the ray."""
    sc = wc.scene(p, s, G64)
    m = (lambda w: w) if s > 0 else (lambda w: 56.0 - w)                        # brick slab 3 mirrored onto itself
    wu, wv = (m(28.0), m(26.6)) if first == "v" else (m(26.6), m(28.0))
    d = (0.5 * su, 0.4 * sv, float(s))
    at = lambda w: np.array([32.0 + d[0] * (w - wu) / d[2], 16.0 + d[1] * (w - wv) / d[2], w])
    order = range(24, 32) if s > 0 else range(31, 23, -1)
    cells = [np.floor(at(c + 0.5)).astype(int) for c in order]                  # the cell the ray is in at the middle of every cell slab, in travel order
    path = []
    for c in cells:
        if brick(c) not in path:
            path.append(brick(c))
    four = [(4, 2), (3, 2), (4, 1), (3, 1)]
    assert len(path) == 3 and path[0] == (4 if su < 0 else 3, 2 if sv < 0 else 1) and path[2] == (3 if su < 0 else 4, 1 if sv < 0 else 2)
    tb = path[target]
    T = sc.add(*next(c for c in cells if brick(c) == tb))                       # the first cell of the path inside the target brick
    later = [sc.add(*[c for c in cells if brick(c) == b][-1]) for b in path[target + 1:]]
    o, dd = ray_along(at(28.0), d, n=1)
    rays = sc.make_rays(o, dd)
    beside = []
    for b in four:
        if b == tb or b in path[target + 1:]:
            continue
        cu, cv = (32 if b[0] == 4 else 31), (16 if b[1] == 2 else 15)            # the brick's cell at the corner
        for cw in order:                                                         # ... in a cell slab where the ray does not touch it
            probe = wc.scene(p, s, G64)
            probe.add(cu, cv, cw)
            if probe.finish(rays).ref_t[0] < 0:
                beside.append(sc.add(cu, cv, cw))
                break
    sc.finish(rays)
    assert len(later) + len(beside) == 3 and len(sc.order) == 4                  # one occupied cell in each of the four bricks
    assert sc.ref_cell[0] == T and sc.ref_t[0] > 0
    assert all(sc.alone(c)[0] > sc.ref_t[0] for c in later) and all(sc.alone(c)[0] < 0 for c in beside)
    return sc


@pytest.mark.parametrize("first,target", QUAD)
@pytest.mark.parametrize("su,sv", SIGNS, ids=["uu", "du", "ud", "dd"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_four_bricks_occupied_ray_through_three(gpu, p, s, su, sv, first, target):
    wc.check(gpu, quad_scene(p, s, su, sv, first, target), shadow=True, big=True)


# ---- 7. far origins: windows of rectangle cells ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_scene(p, s, su, sv):
    """ray_extremes' axial far-origin family aimed at the two voxels of the higher-brick case from about 1.1e7 voxel sizes away: the
    tolerance is above ten voxel sizes, the rectangle some 6 x 5 bricks -- more than one 16-cell window, which keeps index order."""
    base = higher_brick_first_scene(p, s, su, sv)
    lo, hi = base.oa["mn"].min(0).astype(np.float64), base.oa["mx"].max(0).astype(np.float64)
    box = types.SimpleNamespace(lo=lo, hi=hi)
    rays = wc.rx.far_rays(box, 1.1e7 / float(np.linalg.norm(hi - lo)), "axial", 300, 5)
    sc = wc.scene(p, s, G64)
    sc.cells = list(base.order)
    sc.finish(rays, tmax=3e7)
    assert wc.kernel_tol(sc).min() > 10.0 and (sc.ref_t > 0).sum() >= 10
    return sc


@pytest.mark.parametrize("su,sv", DOWN, ids=["down-u", "down-v", "down-both"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_far_origins_windows_keep_index_order(gpu, p, s, su, sv):
    wc.check(gpu, far_scene(p, s, su, sv), big=True)
