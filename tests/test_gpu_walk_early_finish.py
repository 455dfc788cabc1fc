"""GPU tests of k_walk's early finish: right after a lane's exact tests the kernel compares the new best hit with the ta of the NEXT 1-cell
slab in travel order and, when the hit is closer, retires the ray in the same round -- or, when a sibling brick of the same brick slab is
still pending, sends the lane straight to it.  Everything here is a situation in which that decision could go wrong.

The grids are built by hand (Grid.create + set_voxel); the reference is the definition -- the oracle's brute force over the boxes of the
occupied cells (bool_aabbs + trace_brute) -- and t and prim are compared bit for bit through trace (rank epilogue), trace_ex(want=("t",))
and trace_ex(want=("t", "prim", "normal")) (k_rank), under VOXHIP_TRACE_LDS in {unset, 0} x VOXHIP_TRACE_DONATE in {unset, 0}.

Every construction is written once in the walk's own permuted coordinates (u, v, w) -- w the ray's major axis, u and v the axes after it
cyclically, bricks of a brick slab fetched u-fastest -- for travel along +w, and generated for the three major axes and both travel
directions by permuting the axes and mirroring w.  Each case asserts on the CPU, from the brute force, that it is what it claims to be.

Sizes: 64^3 (one block slab, 8^3 bricks); a 16 x 16 x 128 corridor along each axis (two block slabs); 70 000 x 8 x 8 (cell coordinates
beyond 16 bits: the WIDE variant; its cross-section is one brick, so it has the cases without siblings).  Voxel size 1 and origin 0
keep every plane and every mirrored coordinate an exact float, except where a case needs rounded planes and says so."""
import copy
import functools
import os
import types

import numpy as np
import pytest

import oracle
import ray_extremes as rx

pytestmark = pytest.mark.gpu

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
ORIENTATIONS = [(p, s) for p in range(3) for s in (1, -1)]   # (major axis, travel direction along it)
ENVS = [(None, None), (0, None), (None, 0), (0, 0)]          # (VOXHIP_TRACE_LDS, VOXHIP_TRACE_DONATE)
G64 = (64, 64, 64)
CORRIDOR = (16, 16, 128)   # (u, v, w)
WIDE = (8, 8, 70000)


class env:
    """Set the library's run-time switches for the duration of a block (read at every launch); None: unset."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def xyz(p, a):
    """(u, v, w) -> (x, y, z) for major axis p (k_walk's unperm):  p=0: x=w y=u z=v;  p=1: x=v y=w z=u;  p=2: x=u y=v z=w"""
    a = np.asarray(a)
    u, v, w = a[..., 0], a[..., 1], a[..., 2]
    return np.stack([(w, u, v), (v, w, u), (u, v, w)][p], axis=-1)


class Scene:
    """Occupied cells and rays, given in (u, v, w) for travel along +w; stored in (x, y, z) for major axis p and direction s."""

    def __init__(self, p, s, dims_uvw, vs=1.0, org=0.0, mirror=True):
        self.p, self.s, self.duvw = p, s, tuple(dims_uvw)
        self.dim = tuple(int(c) for c in xyz(p, np.array(dims_uvw)))
        self.vs, self.org = F(vs), F(org)
        self.mirror = mirror and s < 0   # (mirror=False: the caller writes the construction for direction s itself)
        self.cells = []

    def lin(self, cu, cv, cw):
        """voxel index of cell (cu, cv, cw)"""
        if self.mirror:
            cw = self.duvw[2] - 1 - cw
        assert 0 <= cu < self.duvw[0] and 0 <= cv < self.duvw[1] and 0 <= cw < self.duvw[2], (cu, cv, cw)
        x, y, z = (int(c) for c in xyz(self.p, np.array([cu, cv, cw])))
        return x + self.dim[0] * (y + self.dim[1] * z)

    def add(self, cu, cv, cw):
        self.cells.append(self.lin(int(cu), int(cv), int(cw)))
        return self.cells[-1]

    def make_rays(self, o, d):
        """origins and directions in cell units (position = org + c * vs), rounded to float32 once"""
        o, d = np.array(o, np.float64).reshape(-1, 3), np.array(d, np.float64).reshape(-1, 3)
        if self.mirror:
            o[:, 2] = self.duvw[2] - o[:, 2]
            d[:, 2] = -d[:, 2]
        o = float(self.org) + o * float(self.vs)
        r = np.ascontiguousarray(np.concatenate([xyz(self.p, o), xyz(self.p, d)], axis=1).astype(F))
        assert np.isfinite(r).all() and np.all(np.argmax(np.abs(r[:, 3:]), axis=1) == self.p)   # w is the major axis of every ray
        return r

    def finish(self, rays, tmax=10000.0):
        """bitmask, boxes and the brute-force reference"""
        X, Y, Z = self.dim
        self.rays, self.tmax = rays, tmax
        self.order = np.unique(np.array(self.cells, np.int64))   # getAabbs lists the occupied cells by ascending voxel index
        self.words = np.zeros((X * Y * Z + 31) // 32, np.uint32)
        np.bitwise_or.at(self.words, self.order >> 5, np.uint32(1) << (self.order & 31).astype(np.uint32))
        self.gi = dict(dim=self.dim, bmin=np.full(3, self.org, F))
        self.oa = oracle.bool_aabbs(self.words, self.gi, self.vs)
        assert len(self.oa) == len(self.order)
        self.ref_t, self.ref_p = oracle.trace_brute(self.oa, rays, tmax=tmax, threads=4)
        self.ref_cell = np.where(self.ref_p != MISS, self.order[np.minimum(self.ref_p, len(self.order) - 1)], -1)
        return self

    def alone(self, lin, rays=None):
        """t of the rays against the box of cell `lin` alone"""
        k = int(np.searchsorted(self.order, lin))
        assert self.order[k] == lin
        return oracle.trace_brute(self.oa[k:k + 1], self.rays if rays is None else rays, tmax=self.tmax, threads=1)[0]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run(gpu, sc, shadow=False, envs=ENVS):
    """build the grid by hand and put the rays through the three query forms under the four switch pairs"""
    X, Y, Z = sc.dim
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, Z, sc.vs, (float(sc.org),) * 3)
    try:
        for i in sc.order.tolist():
            g.set_voxel(i % X, (i // X) % Y, i // (X * Y))
        assert np.array_equal(g.bitmask(), sc.words)
        nhit = int((sc.ref_t > 0).sum())
        for lds, don in envs:
            what = (sc.p, sc.s, lds, don)
            with env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=don):
                t, p, nh = g.trace(sc.rays, tmax=sc.tmax)
                assert same_bits(t, sc.ref_t) and np.array_equal(p, sc.ref_p) and nh == nhit, what
                k = g.trace_ex(sc.rays, tmax=sc.tmax, want=("t",))
                assert same_bits(k["t"], sc.ref_t), what
                k = g.trace_ex(sc.rays, tmax=sc.tmax, want=("t", "prim", "normal"))
                assert same_bits(k["t"], sc.ref_t) and np.array_equal(k["prim"], sc.ref_p), what
                if shadow:
                    sh = g.trace_ex(sc.rays, tmax=sc.tmax, any_hit=True, want=("shadowed",))["shadowed"]
                    assert np.array_equal(sh != 0, sc.ref_t > 0), what
    finally:
        g.free()


def bundle(centre, d, back, n=6, seed=0):
    """n rays through `centre`: the first along d exactly, the others with d jittered a little; origins `back` units of d before it"""
    rng = np.random.default_rng(seed)
    dd = np.tile(np.array(d, np.float64), (n, 1))
    dd[1:, :2] += rng.uniform(-0.004, 0.004, size=(n - 1, 2))
    return np.array(centre, np.float64) - back * dd, dd


# ---- 1. the hit is in the last cell slab of its brick --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def last_slab_scene(p, s, dims, kw, behind):
    """Hit cell H = (3, 4, kw), kw the last cell slab of its brick in travel order; behind: None, "brick" (an occupied cell one cell
    further, in the next brick slab) or "block" (one 64 cells further, in the next block slab), both on the ray."""
    sc = Scene(p, s, dims)
    d = (0.03, 0.02, 1.0)
    centre = np.array([3.5, 4.5, kw + 0.5])
    assert kw % 8 == 7 and dims[2] % 8 == 0
    H = sc.add(3, 4, kw)
    B = None
    if behind:
        step = 1 if behind == "brick" else 64
        q = np.floor(centre + step * np.array(d)).astype(int)
        assert q[2] == kw + step and (q[2] >> 3) != (kw >> 3) and ((q[2] >> 6) != (kw >> 6)) == (behind == "block")
        B = sc.add(*q)
    o, dd = bundle(centre, d, 20.0)
    sc.finish(sc.make_rays(o, dd))
    assert sc.ref_cell[0] == H and sc.ref_t[0] > 0 and np.all(sc.ref_cell == H)   # the nearer voxel is the answer
    if B is not None:
        assert sc.alone(B)[0] > sc.ref_t[0]                                         # the ray does go on into the cell behind
    return sc


@pytest.mark.parametrize("behind", [None, "brick", "block"])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_hit_in_last_cell_slab_of_brick(gpu, p, s, behind):
    run(gpu, last_slab_scene(p, s, CORRIDOR, 47, behind), shadow=True)


@pytest.mark.parametrize("behind", [None, "brick", "block"])
@pytest.mark.parametrize("s", [1, -1])
def test_hit_in_last_cell_slab_of_brick_wide(gpu, s, behind):
    """the WIDE variant: cell coordinates beyond 16 bits (travelling along -x the mirrored cells lie below 65536; the variant is the grid's)"""
    run(gpu, last_slab_scene(0, s, WIDE, 65735, behind), shadow=True)


# ---- 2. a sibling brick holds the nearer hit ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sibling_scene(p, s):
    """Brick slab 3 (w in [24, 32)); the ray goes down in u and crosses the brick boundary u = 32 at w = 28: it is in the brick of HIGHER u
    index first, where cell (33, 19, 25) is, and in the brick of lower index -- fetched first -- afterwards, where cell (30, 19, 30) is."""
    sc = Scene(p, s, G64)
    near, far = sc.add(33, 19, 25), sc.add(30, 19, 30)
    assert (33 >> 3) > (30 >> 3) and (25 >> 3) == (30 >> 3)                          # higher brick index, same brick slab, earlier cell slab
    o, dd = bundle((32.0, 19.5, 28.0), (-0.5, 0.01, 1.0), 18.0)
    sc.finish(sc.make_rays(o, dd))
    assert sc.ref_cell[0] == near and sc.alone(far)[0] > sc.ref_t[0] > 0             # both are hit, the one in the higher brick first
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_sibling_brick_holds_nearer_hit(gpu, p, s):
    run(gpu, sibling_scene(p, s), shadow=True)


QUAD = [(first, k) for first in "vu" for k in range(3)]   # which boundary the ray crosses first, and the brick of its path that holds the nearest hit


@functools.lru_cache(maxsize=None)
def quad_scene(p, s, first, target):
    """The 2 x 2 form: the ray goes down in u and in v and crosses u = 32 and v = 16 inside brick slab 3, one at w = 26.6 and the other at
    w = 28, so its path runs through three of the four bricks around that corner (the two orders together reach all four).  The brick
    `target` of the path holds the nearest hit; every later brick of the path holds a farther one; the remaining bricks hold an occupied
    cell beside the ray, at the corner."""
    sc = Scene(p, s, G64)
    wu, wv = (28.0, 26.6) if first == "v" else (26.6, 28.0)
    at = lambda w: np.array([32.0 - 0.5 * (w - wu), 16.0 - 0.4 * (w - wv), w])
    cells = [np.floor(at(c + 0.5)).astype(int) for c in range(24, 32)]               # the cell the ray is in at the middle of every cell slab
    brick = lambda c: (int(c[0]) >> 3, int(c[1]) >> 3)
    path = []
    for c in cells:
        if brick(c) not in path:
            path.append(brick(c))
    assert len(path) == 3 and path[0] == (4, 2) and path[2] == (3, 1)
    tb = path[target]
    tcell = next(c for c in cells if brick(c) == tb)                                 # the first cell of the path inside the target brick
    T = sc.add(*tcell)
    later = [sc.add(*[c for c in cells if brick(c) == b][-1]) for b in path[target + 1:]]
    o, dd = bundle(at(28.0), (-0.5, -0.4, 1.0), 18.0, n=1)
    rays = sc.make_rays(o, dd)
    beside = []
    for b in [(4, 2), (3, 2), (4, 1), (3, 1)]:
        if b == tb or b in path[target + 1:]:
            continue
        cu, cv = (32 if b[0] == 4 else 31), (16 if b[1] == 2 else 15)               # the brick's cell at the corner
        for cw in range(24, 32):                                                     # ... in a cell slab where the ray does not touch it
            probe = Scene(p, s, G64)
            probe.add(cu, cv, cw)
            if probe.finish(rays).ref_t[0] < 0:
                beside.append(sc.add(cu, cv, cw))
                break
    sc.finish(rays)
    assert len(later) + len(beside) == 3 and len(sc.order) == 4                      # one occupied cell in each of the four bricks
    assert sc.ref_cell[0] == T and sc.ref_t[0] > 0
    assert all(sc.alone(c)[0] > sc.ref_t[0] for c in later) and all(sc.alone(c)[0] < 0 for c in beside)
    return sc


@pytest.mark.parametrize("first,target", QUAD)
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_nearest_hit_in_each_of_four_bricks(gpu, p, s, first, target):
    run(gpu, quad_scene(p, s, first, target), shadow=True)


def test_quad_cases_reach_all_four_bricks():
    seen = set()
    for first, target in QUAD:
        sc = quad_scene(2, 1, first, target)
        c = int(sc.ref_cell[0])
        seen.add(((c % 64) >> 3, ((c // 64) % 64) >> 3))
    assert seen == {(4, 2), (3, 2), (4, 1), (3, 1)}


FEW_BELOW = 1_064_960   # launch_walk: a batch below this many rays takes the kernel with four steps per round, from it on the one with two


@pytest.mark.parametrize("n", [FEW_BELOW - 1, FEW_BELOW])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_both_sides_of_the_steps_per_round_threshold(gpu, p, s, n):
    """every other case of this file is a small batch; the sibling case again as a batch on either side of the size at which the launch
    changes kernels (the rays repeated; what a ray returns does not depend on where in the batch it stands)"""
    base = sibling_scene(p, s)
    idx = np.arange(n) % len(base.rays)
    sc = copy.copy(base)
    sc.rays, sc.ref_t, sc.ref_p, sc.ref_cell = np.ascontiguousarray(base.rays[idx]), base.ref_t[idx], base.ref_p[idx], base.ref_cell[idx]
    run(gpu, sc, shadow=True, envs=[ENVS[0], ENVS[3]])


# ---- 3. the check must decline ---------------------------------------------------------------------------------------------------------
def next_slab_ta(sc, ray, k):
    """the kernel's ta of the 1-cell slab behind slab k in travel order, in float32 (walk_step's expression), and its tolerance"""
    o, d = ray[:3], ray[3:]
    hi = np.array(sc.dim, F) * sc.vs + sc.org
    Mx = max(np.abs(o).max(), abs(sc.org), np.abs(hi).max())
    tol = F(Mx) * F(rx.TOL_FACTOR)
    iw, ow = F(1.0) / d[sc.p], o[sc.p]
    if iw > 0:
        return iw * (((sc.org + F(k + 1) * sc.vs) - tol) - ow), tol
    return iw * (((sc.org + F(k) * sc.vs) + tol) - ow), tol


@functools.lru_cache(maxsize=None)
def grazing_scene(p, s, kw):
    """The ray enters the hit cell (20, 19, kw) through its side face u = 20 about 1e-6 voxel sizes in front of the cell's far w plane, and
    the cell directly behind is occupied: the two entry times differ by about 1e-6, far less than the slab tolerance, so best < ta of
    the next slab does NOT hold and the old path has to decide.  Written per direction (no mirror): the far plane is w = kw + 1 or kw,
    and kw is small so that 1e-6 is a few ulps there."""
    sc = Scene(p, s, G64, mirror=False)
    H, B = sc.add(20, 19, kw), sc.add(20, 19, kw + s)
    wf = kw + 1 if s > 0 else kw
    we = wf - s * 1e-6
    o = np.array([[20.0 - 0.5 * 1.5, 19.5 - 0.01 * 1.5, we - s * 1.5]])
    sc.finish(sc.make_rays(o, np.array([[0.5, 0.01, float(s)]])))
    tH, tB = sc.alone(H)[0], sc.alone(B)[0]
    assert sc.ref_cell[0] == H and 0 < tH < tB and tB - tH < 3e-6, (tH, tB)
    ta, tol = next_slab_ta(sc, sc.rays[0], kw)
    assert not (tH < ta) and tB - tH < tol                                           # the check has nothing to say here
    return sc


@pytest.mark.parametrize("kw", [1, 7, 8])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_grazing_entry_in_front_of_far_plane(gpu, p, s, kw):
    """kw = 1: the cell behind is in the same brick; 7 (+w) and 8 (-w): the hit is in the brick's last cell slab and the cell behind in
    the next brick slab; 8 (+w) and 7 (-w): the brick's first cell slab"""
    run(gpu, grazing_scene(p, s, kw))


@functools.lru_cache(maxsize=None)
def tie_scene(p, s):
    """The exact tie: two cells adjacent along w, the ray in through their shared edge (the side plane u = const where it meets the plane
    between them).  With exact planes the first cell's exit time IS the second's entry time and only one of them can report the side
    plane's time; so this grid has voxel size 0.1 and origin 0.3, where for some k the rounded box planes overlap by an ulp
    (max_w of cell k > min_w of cell k + 1), and the rays are searched, a few ulps around the aim, for those whose side-plane time falls
    into that overlap: both boxes then report exactly that float, and the lower voxel index wins."""
    col = Scene(p, s, G64, vs=0.1, org=0.3, mirror=False)
    cu, cv = 20, 19
    for k in range(64):
        col.add(cu, cv, k)
    col.finish(np.ones((1, 6), F))                                                   # (only the boxes are wanted)
    mn, mx = col.oa["mn"].astype(np.float64), col.oa["mx"].astype(np.float64)      # ascending voxel index = ascending k
    pu, pv = (p + 1) % 3, (p + 2) % 3
    ks = [k for k in range(2, 61) if mx[k, p] > mn[k + 1, p]]
    assert ks, "no overlapping pair of planes on this grid"
    Pu, vc = mn[0, pu], 0.5 * (mn[0, pv] + mx[0, pv])
    ulp = float(np.spacing(F(Pu)))
    o, d, pair = [], [], []
    for k in ks[:12]:
        lo, hi = mn[k + 1, p], mx[k, p]                                              # the overlap [lo, hi] along w
        for T in (1.5, 1.25, 1.75, 1.375):
            ow = (lo - T) if s > 0 else (hi + T)
            for j in range(-8, 9):
                w3 = np.zeros(3)
                w3[p], w3[pu], w3[pv] = ow, Pu - 0.5 * T + 0.5 * j * ulp, vc - 0.001 * T
                d3 = np.zeros(3)
                d3[p], d3[pu], d3[pv] = float(s), 0.5, 0.001
                o.append(w3), d.append(d3), pair.append(k)
    cand = np.ascontiguousarray(np.concatenate([np.array(o), np.array(d)], axis=1).astype(F))
    pair = np.array(pair)
    t0, t1 = np.zeros(len(cand), F), np.zeros(len(cand), F)
    for k in np.unique(pair):
        m = pair == k
        t0[m] = oracle.trace_brute(col.oa[k:k + 1], cand[m], threads=1)[0]
        t1[m] = oracle.trace_brute(col.oa[k + 1:k + 2], cand[m], threads=1)[0]
    tie = np.flatnonzero((t0 > 0) & (t0 == t1))
    assert len(tie), "no ray with equal t on both cells found"
    k = int(pair[tie[0]])
    tie = tie[pair[tie] == k][:8]
    sc = Scene(p, s, G64, vs=0.1, org=0.3, mirror=False)
    a, b = sc.add(cu, cv, k), sc.add(cu, cv, k + 1)
    sc.finish(np.ascontiguousarray(cand[tie]))
    assert np.array_equal(sc.alone(a), sc.alone(b)) and same_bits(sc.ref_t, sc.alone(a)) and np.all(sc.ref_t > 0)
    assert np.all(sc.ref_cell == min(a, b))
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_exact_tie_across_two_cell_slabs(gpu, p, s):
    run(gpu, tie_scene(p, s))


# ---- 4. split rays ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corridor_scene(p, s, n):
    """An end wall behind 127 empty cell slabs and one voxel S halfway.  Of every four rays one points away from the grid (it retires at
    refill, so 48 lanes of every wave are busy -- the donation threshold -- and the static chunks cover the batch: the waves start
    drained and cut their rays at once), one is aimed through S, two at the wall."""
    sc = Scene(p, s, CORRIDOR)
    for cu in range(16):
        for cv in range(16):
            sc.add(cu, cv, 127)
    S = sc.add(8, 8, 64)
    rng = np.random.default_rng(100 + n)
    o = np.concatenate([rng.uniform(1.0, 15.0, size=(n, 2)), np.full((n, 1), 0.5)], axis=1)
    tgt = np.concatenate([rng.uniform(1.0, 15.0, size=(n, 2)), np.full((n, 1), 127.5)], axis=1)
    stop = np.arange(n) % 4 == 1
    o[stop, :2] = rng.uniform(3.0, 13.0, size=(stop.sum(), 2))                        # (so that behind S the ray stays inside the corridor)
    tgt[stop] = np.concatenate([rng.uniform(8.2, 8.8, size=(stop.sum(), 2)), np.full((stop.sum(), 1), 64.5)], axis=1)
    d = tgt - o
    away = np.arange(n) % 4 == 0
    o[away, 2] = -5.0
    d[away] = (0.01, 0.01, -1.0)
    sc.finish(sc.make_rays(o, d))
    assert np.all(sc.ref_t[away] < 0) and np.all(sc.ref_cell[stop] == S) and np.all(sc.ref_t[~away] > 0)
    assert (sc.ref_cell[~away & ~stop] != S).sum() >= n // 4                          # rays that go all the way to the wall
    # the far piece of a ray that stops at S would find the wall: without S every such ray hits it, farther away
    kS = int(np.searchsorted(sc.order, S))
    tw = oracle.trace_brute(np.delete(sc.oa, kS), sc.rays[stop], threads=4)[0]
    assert np.all(tw > sc.ref_t[stop])
    return sc


@pytest.mark.parametrize("n", [64, 256, 4096])
@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_split_rays_down_the_corridor(gpu, p, s, n):
    run(gpu, corridor_scene(p, s, n))


# ---- 5. far origins --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_scene(p, s):
    """ray_extremes' axial far-origin family aimed at the two voxels of the sibling case, from about 1.1e7 voxel sizes away: tol is above
    10 voxel sizes, so around the voxels (u about 32, v about 19) the slab rectangle spans at least [12, 52] x [0, 39] cells -- 6 x 5
    bricks, more than one 16-cell window (pend bit 31)."""
    base = sibling_scene(p, s)
    lo, hi = base.oa["mn"].min(0).astype(np.float64), base.oa["mx"].max(0).astype(np.float64)
    box = types.SimpleNamespace(lo=lo, hi=hi)
    D = 1.1e7 / float(np.linalg.norm(hi - lo))
    rays = rx.far_rays(box, D, "axial", 300, 5)
    sc = Scene(p, s, G64)
    sc.cells = list(base.order)
    sc.finish(rays, tmax=3e7)                                                         # (the rays are unit vectors: t is about 1.1e7)
    tol = np.abs(rays[:, :3]).max(axis=1) * F(rx.TOL_FACTOR)
    assert tol.min() > 10.0 and (sc.ref_t > 0).sum() >= 10, (tol.min(), int((sc.ref_t > 0).sum()))
    return sc


@pytest.mark.parametrize("p,s", ORIENTATIONS)
def test_far_origins_need_more_than_one_window(gpu, p, s):
    run(gpu, far_scene(p, s))
