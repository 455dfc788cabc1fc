"""Ray generators, scene fixtures and reference wrappers for the ray regimes the ordinary generators never reach: origins far from the
scene, directions scaled by powers of two, subnormal direction components and the edges of the ray interval.  A helper for
tests/test_ray_extremes_cpu.py and tests/test_gpu_ray_extremes.py, not a test itself.

Every ray is built in float64 and rounded to float32 once; all components stay finite (only tmax and per-ray tmax may be +inf).
Scenes, rays and reference results are cached per process: every test of a module shares one copy and leaves it unchanged."""
import functools
import types

import numpy as np

import instance_ref
import mesh_multihit_ref as mmr
import mesh_ref
import multihit_ref as mr
import oracle
import vx_scenes

F = np.float32
INF = F(np.inf)
FLT_MAX = np.finfo(np.float32).max
MISS = np.uint32(0xFFFFFFFF)
K_SCALES = (-100, -40, 0, 40, 100)
K_MULTI = 4
N_MULTI_WIDE = 20                         # multi-hit on the 860 430-box grid: the reference is a rays x boxes matrix, so fewer rays of each family
TOL_FACTOR = 9.5367431640625e-07          # walk_setup: tol = 16 * 2^-24 * max |coordinate| over the ray origin and the grid corners

GRID_SCENES = ("rotcube", "adversarial", "wide")
BVH_SCENES = ("floor", "adversarial")
# Far-origin families (D, shape) per scene: origin = centre + D * diagonal * s.  A pair stays only where the reference itself still hits at
# least HIT_FLOOR of the rays (tests/test_ray_extremes_cpu.py asserts it).  Beyond that the float32 formula has nothing left to find: on
# the grids at D = 1e7 hitAabb's `plane - origin` rounds every box of the scene to the same entry and exit time, and on the wide grid, whose
# own extent is 10^5, a diagonal origin at D >= 1e3 no longer finds the 8 x 8-cell cross-section through a rounded direction -- so the wide
# grid takes its diagonal rays at D = 1e2 (10^7 voxel sizes away, tol = 5.6 voxels) and its axial ones at D = 1e3 and 1e5.
_BOTH = ("diagonal", "axial")
_TO_1E6 = [(D, s) for D in (1e3, 1e5, 1e6) for s in _BOTH]
_TO_1E7 = [(D, s) for D in (1e3, 1e5, 1e6, 1e7) for s in _BOTH]
FAR_KEYS = {("grid", "rotcube"): _TO_1E6, ("grid", "adversarial"): _TO_1E6, ("grid", "wide"): [(1e2, "diagonal"), (1e3, "axial"), (1e5, "axial")],
            ("bvh", "floor"): _TO_1E7, ("bvh", "adversarial"): _TO_1E7, ("tlas", "tlas"): _TO_1E7}
HIT_FLOOR = 0.2
N_RAYS = {("grid", "rotcube"): 2000, ("grid", "adversarial"): 2000, ("grid", "wide"): 160, ("bvh", "floor"): 3000, ("bvh", "adversarial"): 1500,
          ("tlas", "tlas"): 800}


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_scene(name):
    """rotcube at 0.09 (32 x 31 x 37), adversarial at 0.0625, and the 100 000 x 8 x 8 grid that selects k_walk's WIDE variants"""
    if name == "wide":
        from test_gpu_parity import long_thin_mesh
        v, t = long_thin_mesh()
        vs = F(1.0)
    else:
        v, t = vx_scenes.scene(name)
        vs = F({"rotcube": 0.09, "adversarial": 0.0625}[name])
    ow, _, gi = oracle.build_bool(v, t, vs, threads=4)
    oa = oracle.bool_aabbs(ow, gi, vs)
    lo = gi["bmin"].astype(np.float64)
    hi = lo + np.array(gi["dim"], np.float64) * float(vs)
    gi = {"dim": gi["dim"], "bmin": gi["bmin"], "bmax": hi.astype(F)}
    return _ns(name=name, v=v, t=t, vs=vs, ow=ow, gi=gi, oa=oa, lo=lo, hi=hi)


@functools.lru_cache(maxsize=None)
def mesh_scene(name):
    """floor: the cube on two axis-aligned floor triangles (zero-thickness boxes); adversarial: slivers on the ill-conditioned side list"""
    if name == "floor":
        from test_gpu_mesh_trace import floor_scene
        v, t = floor_scene()
    else:
        v, t = vx_scenes.scene(name)
    v, t = np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32)
    return _ns(name=name, v=v, t=t, lo=v.min(0).astype(np.float64), hi=v.max(0).astype(np.float64))


@functools.lru_cache(maxsize=None)
def tlas_scene():
    """8 instances of two meshes: uniformly scaled, non-uniformly scaled, mirrored, sheared, and one translated by 10^3"""
    rng = np.random.default_rng(8)
    meshes = [tuple(np.ascontiguousarray(a) for a in vx_scenes.scene("rotcube")), tuple(np.ascontiguousarray(a) for a in vx_scenes.blob(nlon=24, nlat=20))]
    rot = [instance_ref.random_rotation(rng) for _ in range(8)]
    tr = [instance_ref.transform(rot[0], (1.7, 1.7, 1.7), 0.0, (-3.0, 0.5, 1.0)),          # uniform scale
          instance_ref.transform(rot[1], (0.4, 2.5, 1.1), 0.0, (2.5, -1.0, -2.0)),         # non-uniform scale
          instance_ref.transform(rot[2], (-1.3, 0.8, 1.2), 0.0, (0.5, 3.0, 2.5)),          # mirrored: det < 0
          instance_ref.transform(rot[3], (1.0, 1.0, 1.0), 0.0, (1000.0, 2.0, -1.0)),       # translated by 10^3
          instance_ref.transform(rot[4], (0.9, 1.4, 0.6), 0.5, (-1.0, -3.0, -0.5)),        # sheared
          instance_ref.transform(np.eye(3), (1.0, 1.0, 1.0), 0.0, (0.0, 0.0, 0.0)),
          instance_ref.transform(rot[6], (2.0, 2.0, 2.0), 0.0, (3.5, 2.0, -3.5)),
          instance_ref.transform(rot[7], (1.2, -0.7, 1.5), 0.0, (-3.5, 2.5, -3.0))]
    inst = instance_ref.make_instances(tr, blas=[0, 1, 0, 1, 0, 1, 1, 0])
    boxes = []
    for i in range(len(inst)):
        p = instance_ref.world_vertices(inst["transform"][i], meshes[int(inst["blas"][i])][0]).astype(np.float64)
        boxes.append((p.min(0), p.max(0)))
    blo, bhi = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    return _ns(name="tlas", meshes=meshes, inst=inst, blo=blo, bhi=bhi, lo=blo.min(0), hi=bhi.max(0))


def scene_of(kind, name):
    return {"grid": grid_scene, "bvh": mesh_scene}[kind](name) if kind != "tlas" else tlas_scene()


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def _rays(o32, d64):
    """origins already float32; directions rounded once, a component that rounds to zero replaced as the ordinary generators do"""
    d = np.asarray(d64, np.float64).astype(F)
    d[d == 0] = F(1e-20)
    r = np.ascontiguousarray(np.concatenate([o32, d], axis=1), dtype=F)
    assert np.isfinite(r).all()
    return r


def _targets(sc, n, rng):
    """uniform in the scene's box; for the instanced scene uniform in the world box of a random instance (the scene's own box is empty
    but for a few parts in 10^3 of its length)"""
    if hasattr(sc, "blo"):
        k = rng.integers(0, len(sc.blo), n)
        return rng.uniform(sc.blo[k], sc.bhi[k])
    return rng.uniform(sc.lo, sc.hi, size=(n, 3))


def far_rays(sc, D, shape, n, seed):
    """Family 1: o = c + D * L * s, d = normalise(target - o); shape "diagonal": s uniform on the sphere; "axial": s one signed
    coordinate axis and the other two origin components inside the box"""
    rng = np.random.default_rng(seed)
    c, L = (sc.lo + sc.hi) / 2, float(np.linalg.norm(sc.hi - sc.lo))
    tgt = _targets(sc, n, rng)
    if shape == "diagonal":
        s = rng.normal(size=(n, 3))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        o = c + D * L * s
    else:
        o = rng.uniform(sc.lo, sc.hi, size=(n, 3))
        ax = rng.integers(0, 3, n)
        o[np.arange(n), ax] = c[ax] + rng.choice([-1.0, 1.0], n) * D * L
    o32 = o.astype(F)
    d = tgt - o32.astype(np.float64)
    return _rays(o32, d / np.linalg.norm(d, axis=1, keepdims=True))


def far_keys(kind, name):
    return list(FAR_KEYS[kind, name])


@functools.lru_cache(maxsize=None)
def far_family(kind, name, D, shape):
    n = N_RAYS[kind, name]
    if kind == "grid" and D >= 1e6:
        n //= 2                             # the window regime is slow by design: fewer rays, not a smaller D
    return _frozen(far_rays(scene_of(kind, name), D, shape, n, int(np.log10(D)) * 10 + (shape == "axial")))


@functools.lru_cache(maxsize=None)
def base_rays(kind, name):
    """the suite's ordinary rays: random_rays plus lattice-corner rays (grids) or vertex / edge-midpoint rays (meshes)"""
    sc = scene_of(kind, name)
    n = N_RAYS[kind, name] // 2
    if kind == "grid":
        from test_gpu_parity import corner_rays
        parts = [vx_scenes.random_rays(n, sc.gi["bmin"], sc.gi["bmax"], seed=81), corner_rays(sc.gi, float(sc.vs), n, 82)]
    elif kind == "bvh":
        from test_gpu_mesh_trace import vertex_rays
        parts = [vx_scenes.random_rays(n, sc.lo, sc.hi, seed=83), vertex_rays(sc.v, sc.t, n, 84)]
    else:
        from test_gpu_mesh_trace import vertex_rays
        near = np.arange(len(sc.blo)) != 3
        v, t = sc.meshes[0]
        wv = instance_ref.world_vertices(sc.inst["transform"][0], v)
        parts = [vx_scenes.random_rays(n, sc.blo[near].min(0), sc.bhi[near].max(0), seed=85), vx_scenes.random_rays(n // 2, sc.blo[3], sc.bhi[3], seed=86),
                 vertex_rays(wv, t, n // 2, 87)]
    r = np.concatenate(parts)
    assert (r[:, 3:] != 0).all() and np.isfinite(r).all()
    return _frozen(np.ascontiguousarray(r, F))


@functools.lru_cache(maxsize=None)
def scaled_family(kind, name, k):
    """Family 2: the ordinary rays with d * 2^k (exact: no component leaves the normal range)"""
    r = base_rays(kind, name).copy()
    r[:, 3:] = np.ldexp(r[:, 3:], k)
    tiny = np.finfo(F).tiny
    assert np.isfinite(r).all() and (np.abs(r[:, 3:]) >= tiny).all()
    return _frozen(r)


def _zero_rays(kind, name, n, seed):
    """rays with one or two exactly-zero direction components, origins on and between lattice planes or at mesh vertex coordinates"""
    sc = scene_of(kind, name)
    if kind == "grid":
        from test_gpu_configs import zero_component_rays
        return zero_component_rays(sc.oa, sc.gi, sc.vs, n, seed)
    from test_gpu_mesh_trace import mesh_gi
    from test_gpu_octree_trace import zero_component_rays
    rng = np.random.default_rng(seed + 1)
    if kind == "bvh":
        gi, vs = mesh_gi(sc.v)
        verts = sc.v
    else:
        near = np.arange(len(sc.blo)) != 3
        lo, hi = sc.blo[near].min(0).astype(F), sc.bhi[near].max(0).astype(F)
        gi, vs = mesh_gi(np.stack([lo, hi]))
        verts = np.concatenate([instance_ref.world_vertices(sc.inst["transform"][i], sc.meshes[int(sc.inst["blas"][i])][0]) for i in np.flatnonzero(near)])
    r = zero_component_rays(gi, vs, n, seed)
    vert = verts[rng.integers(0, len(verts), n)]
    at_vertex = (np.arange(n) % 2 == 0)[:, None] & (r[:, 3:] == 0)      # the constant coordinates of every other ray: a vertex's
    r[:, :3] = np.where(at_vertex, vert, r[:, :3])
    return r


@functools.lru_cache(maxsize=None)
def subnormal_family(kind, name, which):
    """Family 3: every zero component replaced by a subnormal, both signs.  "finite": magnitude m * 2^-149 with 2^21 < m < 2^23, whose
    float32 reciprocal is finite; "infinite": 0 < m <= 2^21 (2^-128 and below), whose reciprocal rounds to infinity.  The boundary
    values m = 2^21 + 1, 2^23 - 1 and m = 2^21, 2^20, 1 are always among them."""
    r = _zero_rays(kind, name, N_RAYS[kind, name] // 2, 91 if which == "finite" else 92).copy()
    rng = np.random.default_rng(93 + (which == "finite"))
    z = r[:, 3:] == 0
    nz = int(z.sum())
    if which == "finite":
        m = rng.integers(2 ** 21 + 1, 2 ** 23, nz)
        m[:: 7] = 2 ** 21 + 1
        m[3:: 7] = 2 ** 23 - 1
    else:
        m = rng.integers(1, 2 ** 21 + 1, nz)
        m[:: 7] = 2 ** 21
        m[2:: 7] = 2 ** 20
        m[4:: 7] = 1
    sign = np.where(np.signbit(r[:, 3:][z]) ^ (rng.random(nz) < 0.5), np.uint32(0x80000000), np.uint32(0))
    d = r[:, 3:].copy()
    d[z] = (m.astype(np.uint32) | sign).view(F)
    r[:, 3:] = d
    sub = np.abs(r[:, 3:][z])
    with np.errstate(over="ignore", divide="ignore"):
        assert (sub > 0).all() and (sub < np.finfo(F).tiny).all() and np.isinf(F(1) / sub).all() == (which != "finite")
        assert np.isfinite(F(1) / sub).all() == (which == "finite")
    return _frozen(np.ascontiguousarray(r, F))


@functools.lru_cache(maxsize=None)
def interval_rays(kind, name):
    """Family 4 runs on the ordinary rays plus rays that start inside the scene (so that tmin <= 0 has hits behind it to reject)"""
    from test_gpu_parity import inside_rays
    sc = scene_of(kind, name)
    base = base_rays(kind, name)
    n = len(base) // 3
    gi = {"dim": (1, 1, 1), "bmin": sc.lo.astype(F)}
    ins = inside_rays(gi, 1.0, n, 95)
    rng = np.random.default_rng(96)
    if hasattr(sc, "blo"):
        k = rng.integers(0, len(sc.blo), n)
        ins[:, :3] = rng.uniform(sc.blo[k], sc.bhi[k]).astype(F)
    else:
        ins[:, :3] = rng.uniform(sc.lo, sc.hi, size=(n, 3)).astype(F)
    return _frozen(np.ascontiguousarray(np.concatenate([base[:: 2], ins]), F))


SCALAR_INTERVALS = ((0.0, np.inf), (-1.0, np.inf), (-np.inf, np.inf), (0.0, FLT_MAX), (-1.0, FLT_MAX), (-np.inf, FLT_MAX))
EMPTY_INTERVALS = ((5.0, 1.0), (np.inf, 0.0), (FLT_MAX, 10000.0))          # tmin > tmax: every ray misses


def per_ray_tmax_cases(tstar):
    """per-ray tmax arrays built from the closest hit time t* of [0, +inf] (-1 on a miss): name -> float32 [n]"""
    n = len(tstar)
    hit = tstar > 0
    at = np.where(hit, tstar, INF).astype(F)
    below = np.where(hit, np.nextafter(tstar, F(0), dtype=F), INF).astype(F)
    cases = {"zero": np.zeros(n, F), "minus_one": np.full(n, F(-1)), "t_star": at, "below_t_star": below, "inf": np.full(n, INF)}
    mix = np.stack(list(cases.values()))[np.arange(n) % 5, np.arange(n)]
    cases["mixed"] = np.ascontiguousarray(mix, F)
    return cases


# ---- references -----------------------------------------------------------------------------------------------------------------------
def grid_closest_per_ray(times, tmin, tmax_per_ray):
    """closest hit of the grid contract from a multihit_ref.hit_times matrix, with a per-ray tmax (oracle.trace_brute takes a scalar one):
    the minimum accepted t, ties to the lower box -> (t, prim)"""
    hi = np.asarray(tmax_per_ray, F)[:, None]
    with np.errstate(invalid="ignore"):
        acc = (times > F(0)) & (times >= F(tmin)) & (times <= hi)
    tt = np.where(acc, times, INF).min(axis=1)
    hit = acc.any(axis=1)
    k = np.argmax(acc & (times == tt[:, None]), axis=1)
    return np.where(hit, tt, F(-1)).astype(F), np.where(hit, k.astype(np.uint32), MISS)


def ref_closest(kind, sc, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None, boxes=None):
    """-> dict of the closest-hit outputs of the scene's reference (t, prim; bary for meshes; instance for the instanced scene)"""
    if kind == "grid":
        oa = sc.oa if boxes is None else boxes
        if tmax_per_ray is None:
            t, p = oracle.trace_brute(oa, rays, tmin, tmax)
        else:
            # the accepted set under tmax_r is the part of the accepted set of [tmin, +inf] at or below tmax_r: its minimum is that
            # set's minimum (t, prim) when t <= tmax_r and it is empty otherwise (the CPU test checks this against grid_closest_per_ray)
            t, p = oracle.trace_brute(oa, rays, tmin, np.inf)
            keep = (t > 0) & (t <= np.asarray(tmax_per_ray, F))
            t, p = np.where(keep, t, F(-1)).astype(F), np.where(keep, p, MISS).astype(np.uint32)
        return {"t": t, "prim": p}
    if kind == "bvh":
        t, p, b = mesh_ref.closest(sc.v, sc.t, rays, tmin, tmax, tmax_per_ray)
        return {"t": t, "prim": p, "bary": b}
    t, i, p, b = instance_ref.closest(sc.meshes, sc.inst, rays, tmin, tmax, tmax_per_ray)
    return {"t": t, "instance": i, "prim": p, "bary": b}


def ref_any(kind, sc, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None, boxes=None):
    if kind == "grid":
        return oracle.trace_any_brute(sc.oa if boxes is None else boxes, rays, tmin, tmax, tmax_per_ray)
    if kind == "bvh":
        return mesh_ref.any_hit(sc.v, sc.t, rays, tmin, tmax, tmax_per_ray)
    return instance_ref.any_hit(sc.meshes, sc.inst, rays, tmin, tmax, tmax_per_ray)


def multi_rays(kind, name, fam):
    """the rays of a family that the multi-hit query is run on: all of them, but N_MULTI_WIDE evenly spaced ones on the wide grid"""
    rays = family(kind, name, fam)
    if (kind, name) != ("grid", "wide"):
        return rays
    return _frozen(np.ascontiguousarray(rays[np.linspace(0, len(rays) - 1, N_MULTI_WIDE).astype(int)]))


def ref_multi(kind, sc, rays, tmin=0.001, tmax=10000.0, k=K_MULTI):
    """-> dict of the multi-hit outputs (t, prim, count; bary / instance as above), K = 4"""
    if kind == "grid":
        step = 64 if len(sc.oa) < 100000 else 4          # rays per slice of the rays x boxes x 3 temporaries
        times = np.concatenate([mr.hit_times(sc.oa, rays[s:s + step], chunk=step) for s in range(0, len(rays), step)])
        t, p, c = mr.select(times, k, tmin=tmin, tmax=tmax)
        return {"t": t, "prim": p, "count": c}
    if kind == "bvh":
        out = mmr.select(mmr.all_hits(sc.v, sc.t, rays, tmin, tmax), k)
        out.pop("instance")
        return out
    return mmr.select(mmr.all_hits_tlas(sc.meshes, sc.inst, rays, tmin, tmax), k)


def scaled_t(t, k):
    """t * 2^-k where t is a hit time, the miss marker (-1) kept"""
    t = np.asarray(t, F)
    with np.errstate(over="ignore", under="ignore"):
        return np.where(t > 0, np.ldexp(t, -k), t).astype(F)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == F:
        return a.shape == b.shape and b.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def first_difference(got, ref, rays):
    """a readable account of the first ray on which two output dicts differ (None: they are bit-equal on every shared field)"""
    for f in ref:
        if f not in got:
            continue
        g, r = np.ascontiguousarray(got[f]), np.ascontiguousarray(ref[f])
        if same_bits(g, r):
            continue
        gv, rv = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == F else (g, r)
        bad = np.flatnonzero((gv != rv).reshape(len(gv), -1).any(axis=1))
        i = int(bad[0])
        return "%s differs on %d of %d rays; first ray %d: got %r, reference %r, ray %s" % (f, len(bad), len(gv), i, g[i].tolist(), r[i].tolist(),
                                                                                          [float.hex(float(x)) for x in rays[i]])
    return None


def walk_tol(sc, rays):
    """walk_setup's position tolerance per ray: TOL_FACTOR * max |coordinate| over the ray origin and the grid's corners, float32"""
    corner = F(max(np.abs(sc.gi["bmin"]).max(), np.abs(sc.gi["bmin"] + np.array(sc.gi["dim"], F) * sc.vs).max()))
    return (np.maximum(np.abs(rays[:, :3]).max(axis=1), corner) * F(TOL_FACTOR)).astype(F)


# ---- family 4: the interval cases both test files walk through ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def t_star(kind, name):
    """the closest hit of every interval ray over [0, +inf]: dict of read-only arrays"""
    return reference(kind, name, ("interval",), "closest", 0.0, np.inf)


def exact_cases(kind, name, count=6, batch=256, tstar=None):
    """-> (rays, [(j, t*_j)]): a small batch of interval rays and `count` hitting rays of it whose own t* becomes an interval bound
    (`tstar`: the closest hit times over [0, +inf] of another box list than the scene's own, such as an octree's)"""
    ts = (t_star(kind, name)["t"] if tstar is None else np.asarray(tstar, F))[:batch]
    hits = np.flatnonzero(ts > 0)
    js = hits[np.linspace(0, len(hits) - 1, count).astype(int)]
    return interval_rays(kind, name)[:batch], [(int(j), F(ts[j])) for j in js]


def exact_intervals(ts):
    """the three intervals built on one hit time: closed at both ends on it, open just above it, closed just below it"""
    return {"at": (ts, ts), "above": (np.nextafter(ts, INF, dtype=F), INF), "below": (F(0), np.nextafter(ts, F(0), dtype=F))}


# ---- every (family, interval) with its reference, computed once per process -----------------------------------------------------------------
def family(kind, name, fam):
    """fam = ("far", D, shape) | ("scaled", k) | ("subnormal", which) | ("interval",) | ("exact",) -> the family's rays"""
    if fam[0] == "far":
        return far_family(kind, name, fam[1], fam[2])
    if fam[0] == "scaled":
        return scaled_family(kind, name, fam[1])
    if fam[0] == "subnormal":
        return subnormal_family(kind, name, fam[1])
    if fam[0] == "exact":
        return exact_cases(kind, name)[0]
    return interval_rays(kind, name)


@functools.lru_cache(maxsize=None)
def reference(kind, name, fam, what, tmin=0.001, tmax=10000.0):
    """what = "closest" | "any" | "multi" on the family's rays over [tmin, tmax] -> read-only arrays (a dict, or the shadowed bytes)"""
    sc, rays = scene_of(kind, name), multi_rays(kind, name, fam) if what == "multi" else family(kind, name, fam)
    if what == "any":
        return _frozen(ref_any(kind, sc, rays, tmin, tmax))
    out = ref_closest(kind, sc, rays, tmin, tmax) if what == "closest" else ref_multi(kind, sc, rays, tmin, tmax)
    return {k: _frozen(v) for k, v in out.items()}


# ---- where d * 2^k is exact ------------------------------------------------------------------------------------------------------------------
def _mt_scale_safe(verts, tris, rays, k):
    """Moeller-Trumbore's intermediates that carry a factor of d (d x e2, det, dot(s, p), dot(d, q), their products and partial sums) on
    the UNSCALED rays: a (ray, triangle) pair scales exactly when none of them is non-zero and below 2^(-126 - k + 2) -- that is, when
    multiplying d by 2^k cannot push one of them out of float32's normal range, the only place where a power of two is not exact.  Such a
    pair is accepted at both scales or at neither, with the same u, v and t * 2^-k.  A ray is safe when every pair that does NOT scale
    exactly is rejected at both scales (it contributes to no output either way).  On a collinear or point-sized triangle det is a rounding
    residue or a product of 1e-9-sized edges, and 2^-100 times it is subnormal or 0: a handful of rays that such a triangle accepts."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    safe = np.ones(len(rays), bool)
    if k >= 0:
        return safe
    thr = F(2.0 ** (-126 - k + 2))
    tri = mesh_ref._tris(verts, tris)
    v0, e1, e2 = tri
    nt = v0[0].shape[1]
    scaled = rays.copy()
    scaled[:, 3:] = np.ldexp(rays[:, 3:], k)
    for i, j in mesh_ref._chunks(len(rays), nt, budget=1 << 20):
        o = tuple(rays[i:j, a][:, None] for a in range(3))
        d = tuple(rays[i:j, 3 + a][:, None] for a in range(3))
        vals = []
        with np.errstate(all="ignore"):
            s = tuple(o[a] - v0[a] for a in range(3))
            q = mesh_ref._cross(s, e1)
            p = []
            for a, b in ((1, 2), (2, 0), (0, 1)):
                x, y = d[a] * e2[b], d[b] * e2[a]
                vals += [x, y]
                p.append(x - y)
            vals += p
            for lhs in (e1, s):
                x = [lhs[a] * p[a] for a in range(3)]
                vals += x + [x[0] + x[1], (x[0] + x[1]) + x[2]]
            x = [d[a] * q[a] for a in range(3)]
            vals += x + [x[0] + x[1], (x[0] + x[1]) + x[2]]
            bad = np.zeros((j - i, nt), bool)
            for x in vals:
                ax = np.abs(x)
                bad |= (ax > 0) & (ax < thr)
        accepted = mesh_ref._mt(tri, rays[i:j], F(0), INF)[0] | mesh_ref._mt(tri, scaled[i:j], F(0), INF)[0]
        safe[i:j] = ~(bad & accepted).any(axis=1)
    return safe


@functools.lru_cache(maxsize=None)
def scale_safe(kind, name, k):
    """rays of the scaled family on which the scaling relation is exact (all of them on a grid: 1/d and 1/d * (plane - o) stay normal)"""
    sc, rays = scene_of(kind, name), scaled_family(kind, name, 0)
    if kind == "grid":
        return _frozen(np.ones(len(rays), bool))
    if kind == "bvh":
        return _frozen(_mt_scale_safe(sc.v, sc.t, rays, k))
    safe = np.ones(len(rays), bool)
    w, _ = instance_ref.inverse(sc.inst["transform"])
    for i in range(len(sc.inst)):
        v, t = sc.meshes[int(sc.inst["blas"][i])]
        safe &= _mt_scale_safe(v, t, instance_ref.object_rays(w[i], rays), k)
    return _frozen(safe)
