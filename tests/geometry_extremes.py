"""Mesh generators, scaled scenes, OBJ texts and recorded oracle figures for the geometry regimes the ordinary scenes never reach: vertices
that are NaN or infinite, one finite vertex far away from the rest, and whole scenes scaled by powers of two until the voxelizer's products
leave float32's normal range.  A helper for tests/test_geometry_extremes_cpu.py and tests/test_gpu_geometry_extremes.py, not a test itself
(the rules under test: include/voxhip.h, "geometry at its extremes").

Every family is built over the existing scenes `rotcube`, `adversarial` and `floor`.  Meshes, rays and reference results are cached per
process: every test of a module shares one copy and leaves it unchanged (the arrays are read-only)."""
import functools
import types
import zlib

import numpy as np

import instance_ref
import oracle
import ray_extremes as rx
import vx_scenes

F = np.float32
FLT_MAX = np.finfo(F).max
SCENES = ("rotcube", "adversarial", "floor")
GRID_SCENES = ("rotcube", "adversarial")
BVH_SCENES = ("floor", "adversarial")
VOXEL_SIZE = {"rotcube": F(0.09), "adversarial": F(0.0625), "floor": F(0.25)}      # 32 x 31 x 37, 16^3, 32 x 8 x 32 cells

POISON_BITS = {"+nan": 0x7FC00000, "-nan": 0xFFC00000, "nan_payload": 0x7FC00001, "+inf": 0x7F800000, "-inf": 0xFF800000}
POISON_KINDS = ("coord", "vertex", "triangle", "pair")          # each also as the variant `unreferenced`
# "fltmax": +-FLT_MAX/2, whose extent is FLT_MAX exactly -- finite, but the extent over any voxel size below 1 and the world box of an
# instance scaled by 4 overflow; "fltmax_wide": +-0.75 FLT_MAX, whose extent max - min itself overflows to +Inf
OUTLIERS = ("2^100", "fltmax", "fltmax_wide")
OUTLIER_MAG = {"2^100": F(2.0 ** 100), "fltmax": FLT_MAX / F(2), "fltmax_wide": FLT_MAX * F(0.75)}

# scale exponents per SAT variant (sat 1: the variant with the 1e-8 thresholds) and, of those, the ones the ray queries run at
SCALE_K = {1: (-100, -70, -64, -50, -48, -46, -40, -30, 30, 40), 0: (-30, -28, -26, -24, -20, 30, 40)}
TRACE_K = (-64, -30, 30, 40)
# The CPU oracle's (setVoxel calls, occupied voxels) for scene * 2^k at voxel size * 2^k, recorded from the oracle on the host (DESIGN.md
# section 6r holds the table and says what of it the GPU reproduces).  rotcube at 0.09 * 2^k is 32 x 31 x 37 at every k, adversarial at
# 0.0625 * 2^k 16^3.  The k outside SCALE_K (0, -16, -22, -42, -44, -60) are host figures only: the GPU tests do not run them.
ORACLE_TABLE = {
    ("rotcube", 1): {0: (5022, 4307), 30: (5022, 4307), 40: (5022, 4307), -30: (5022, 4307), -40: (5022, 4307), -42: (5022, 4307), -44: (5022, 4307),
                     -46: (5027, 4312), -48: (5109, 4386), -50: (6803, 6103), -60: (9839, 8851), -64: (9839, 8851), -70: (9929, 8925),
                     -100: (71340, 33504)},
    ("rotcube", 0): {0: (5022, 4307), 30: (5022, 4307), 40: (5022, 4307), -16: (9839, 8851), -20: (9839, 8851), -24: (9839, 8851), -26: (9853, 8863),
                     -28: (18060, 14336), -30: (71340, 33504)},
    ("adversarial", 1): {0: (21261, 3934), 30: (21261, 3934), 40: (21261, 3934), -30: (21261, 3934), -40: (21200, 3934), -42: (21714, 3934),
                         -44: (21764, 3934), -46: (21619, 3936), -48: (21641, 3941), -50: (26992, 3966), -64: (26992, 3966), -70: (27496, 3971),
                         -100: (243200, 4096)},
    ("adversarial", 0): {0: (21307, 3934), 30: (21261, 3934), 40: (21261, 3934), -20: (26992, 3966), -22: (27016, 3966), -24: (27992, 3986),
                         -26: (31338, 4013), -28: (243200, 4096), -30: (243200, 4096)},
}
# the k whose setVoxel-call counts are pairwise distinct: where gradual underflow (and, for sat 1, the 1e-8 thresholds) set in
DISTINCT_K = {("rotcube", 1): (-40, -46, -48, -50, -64, -70, -100), ("rotcube", 0): (-24, -26, -28, -30),
              ("adversarial", 1): (-40, -42, -44, -46, -48, -50), ("adversarial", 0): (-22, -24, -26, -28)}


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def scene(name):
    """(vertices float32[V, 3], triangles int32[T, 3]) of rotcube, adversarial or floor, read-only"""
    if name == "floor":
        from test_gpu_mesh_trace import floor_scene
        v, t = floor_scene()
    else:
        v, t = vx_scenes.scene(name)
    return _frozen(np.asarray(v, F)), _frozen(np.asarray(t, np.int32))


def poison_value(value, flip=False):
    """the float32 with the named bit pattern (flip: its sign bit inverted)"""
    return np.array([POISON_BITS[value] ^ (0x80000000 if flip else 0)], np.uint32).view(F)[0]


def _interleave(t, strays, rng):
    """the stray triangles put in at seeded positions among the real ones -> (triangles, remap): remap[new index] = the clean mesh's
    index of that triangle, -1 for a stray"""
    pos = np.sort(rng.integers(0, len(t) + 1, len(strays)))
    tt = np.insert(np.asarray(t, np.int32), pos, np.asarray(strays, np.int32), axis=0)
    remap = np.insert(np.arange(len(t), dtype=np.int64), pos, -1)
    return _frozen(tt.astype(np.int32)), _frozen(remap)


def _mesh(name, new_verts, strays, rng, referenced):
    v, t = scene(name)
    vv = _frozen(np.concatenate([v, np.asarray(new_verts, F).reshape(-1, 3)]).astype(F))
    if referenced:
        tt, remap = _interleave(t, strays, rng)
    else:
        tt, remap = t, _frozen(np.arange(len(t), dtype=np.int64))
    return _ns(name=name, v=vv, t=tt, clean_v=v, clean_t=t, remap=remap, stray=_frozen(remap < 0), first_new=len(v))


def _edges(t, rng, n):
    """n (a, b) vertex pairs, each an edge of a random triangle of the scene: a stray built on one reaches out of the scene's own surface"""
    tri = np.asarray(t)[rng.integers(0, len(t), n)]
    k = rng.integers(0, 3, n)
    return tri[np.arange(n), k], tri[np.arange(n), (k + 1) % 3]


@functools.lru_cache(maxsize=None)
def poisoned(name, kind, value, referenced=True):
    """The scene plus stray triangles over its own vertices with poisoned coordinates.  kind: "coord" one coordinate of one vertex, "vertex"
    a whole vertex, "triangle" all three vertices of a stray, "pair" -value and +value on the same axis in two strays.  value: a key of
    POISON_BITS.  referenced=False: the same poisoned vertices appended and no triangle using them."""
    v, t = scene(name)
    rng = np.random.default_rng(_seed(name, kind, value))
    p, q = poison_value(value), poison_value(value, flip=True)
    base = v[rng.integers(0, len(v), 3)].copy()
    ax = int(rng.integers(0, 3))
    n0 = len(v)
    a, b = _edges(t, rng, 3)
    if kind == "coord":
        base[0, ax] = p
        new, strays = base[:1], [(a[i], b[i], n0) for i in range(3)]
    elif kind == "vertex":
        base[0, :] = p
        new, strays = base[:1], [(a[i], n0, b[i]) for i in range(3)]
    elif kind == "triangle":
        for i in range(3):
            base[i, (ax + i) % 3] = p
        new, strays = base, [(n0, n0 + 1, n0 + 2), (n0 + 2, n0, n0 + 1)]
    elif kind == "pair":
        base[0, ax], base[1, ax] = q, p
        new, strays = base[:2], [(a[0], b[0], n0), (n0 + 1, a[1], b[1])]
    else:
        raise ValueError(kind)
    m = _mesh(name, new, strays, rng, referenced)
    assert not np.isfinite(m.v[n0:]).all() and np.isfinite(m.v[:n0]).all()
    return m


@functools.lru_cache(maxsize=None)
def outlier(name, mag, referenced=True, seed=0):
    """The same with finite values: "2^100" one vertex with one coordinate at +-2^100 (the extent stays finite); "fltmax" two vertices at
    +FLT_MAX/2 and -FLT_MAX/2 on one axis (max - min = FLT_MAX), "fltmax_wide" at +-0.75 FLT_MAX (max - min overflows to +Inf).  Every stray stands on an edge of the scene and reaches to the
    outlier: v0, v1 the edge, v2 the far vertex."""
    v, t = scene(name)
    rng = np.random.default_rng(_seed(name, mag, seed))
    base = v[rng.integers(0, len(v), 2)].copy()
    ax = int(rng.integers(0, 3))
    n0 = len(v)
    a, b = _edges(t, rng, 8)
    if mag == "2^100":
        base[0, ax] = F(2.0 ** 100) * F(rng.choice([-1.0, 1.0]))
        new, strays = base[:1], [(a[i], b[i], n0) for i in range(8)]
    elif mag in ("fltmax", "fltmax_wide"):
        base[0, ax], base[1, ax] = OUTLIER_MAG[mag], -OUTLIER_MAG[mag]
        new, strays = base, [(a[i], b[i], n0 + (i & 1)) for i in range(8)]
    else:
        raise ValueError(mag)
    m = _mesh(name, new, strays, rng, referenced)
    assert np.isfinite(m.v).all()
    with np.errstate(over="ignore"):
        ext = (m.v.max(0) - m.v.min(0)).max()
        assert np.isfinite(ext) == (mag != "fltmax_wide") and (mag == "2^100" or np.isinf(ext * F(4)))
    return m


@functools.lru_cache(maxsize=None)
def scaled(name, k):
    """scene * 2^k with its voxel size * 2^k.  np.ldexp is exact while the result stays in float32's normal range (or is zero); `exact`
    says whether every coordinate did (the adversarial scene's smallest coordinates go subnormal at k = -100: both sides of every
    comparison read the same rounded input)."""
    v, t = scene(name)
    with np.errstate(under="ignore"):
        vv = np.ldexp(v, k).astype(F)
        vs = np.ldexp(VOXEL_SIZE[name], k).astype(F)
        exact = bool(np.array_equal(np.ldexp(vv, -k).astype(F), v))
    assert np.isfinite(vv).all() and vs > 0 and np.ldexp(vs, -k) == VOXEL_SIZE[name]
    return _ns(name=name, k=k, v=_frozen(vv), t=t, vs=vs, exact=exact)


def scaled_rays(rays, k):
    """origins * 2^k, directions kept: the same geometric ray in the scaled scene (hit times scale by 2^k with the interval)"""
    r = np.array(rays, F)
    r[:, :3] = np.ldexp(r[:, :3], k)
    assert np.isfinite(r).all()
    return _frozen(r)


def scaled_interval(k, tmin=0.001, tmax=10000.0):
    return F(np.ldexp(F(tmin), k)), F(np.ldexp(F(tmax), k))


@functools.lru_cache(maxsize=None)
def outlier_tlas(name, mag):
    """Four instances of the outlier mesh (identity; a rotation; scale 4, whose world box overflows float32 for the "fltmax" kinds; mirrored) and two
    of the clean rotcube -> ns(meshes, inst)"""
    m = outlier(name, mag)
    rng = np.random.default_rng(_seed("tlas", name, mag))
    rot = [instance_ref.random_rotation(rng) for _ in range(2)]
    eye = np.eye(3)
    tr = [instance_ref.transform(eye, (1.0, 1.0, 1.0), 0.0, (0.0, 0.0, 0.0)),
          instance_ref.transform(rot[0], (1.0, 1.0, 1.0), 0.0, (0.5, -0.25, 0.75)),
          instance_ref.transform(eye, (4.0, 4.0, 4.0), 0.0, (1.0, 2.0, -1.0)),
          instance_ref.transform(eye, (-1.0, 1.0, 1.0), 0.0, (-2.0, 0.5, 1.0)),
          instance_ref.transform(rot[1], (1.0, 1.0, 1.0), 0.0, (3.0, 0.0, -2.0)),
          instance_ref.transform(eye, (1.5, 0.75, 1.25), 0.0, (-3.0, 1.0, 2.5))]
    inst = instance_ref.make_instances(tr, blas=[0, 0, 0, 0, 1, 1])
    inst.setflags(write=False)
    return _ns(name=name, mag=mag, meshes=[(m.v, m.t), scene("rotcube")], inst=inst, stray=m.stray)


@functools.lru_cache(maxsize=None)
def tlas_rays(name):
    """world-space rays of the instanced checks: the scene's own rays (instance 0 is the identity) and random rays over the box that holds
    the near parts of all six instances"""
    return _frozen(np.concatenate([mesh_rays(name)[::3], vx_scenes.random_rays(600, F([-8, -8, -8]), F([8, 8, 8]), seed=77)]).astype(F))


# ---- rays -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_rays(name):
    """the rays of the BVH / TLAS checks on a scene: the suite's ordinary rays (random + vertex / edge-midpoint), the zero-component rays and
    the far family (1e6, "diagonal"), at most 3000 in all"""
    if name == "rotcube":
        v, t = scene(name)
        from test_gpu_mesh_trace import vertex_rays
        base = np.concatenate([vx_scenes.random_rays(500, v.min(0), v.max(0), seed=71), vertex_rays(v, t, 500, 72)])
        return _frozen(base.astype(F))
    base = rx.base_rays("bvh", name)
    zero = rx._zero_rays("bvh", name, 400, 73)
    far = rx.far_family("bvh", name, 1e6, "diagonal")[:600]
    r = np.concatenate([base[:2000], zero, far]).astype(F)
    assert len(r) <= 3000 and np.isfinite(r).all()
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def grid_rays(name, n=600):
    """random + lattice-corner rays of the unscaled grid scene"""
    from test_gpu_parity import corner_rays
    sc = rx.grid_scene(name)
    return _frozen(np.concatenate([vx_scenes.random_rays(n // 2, sc.gi["bmin"], sc.gi["bmax"], seed=75), corner_rays(sc.gi, float(sc.vs), n // 2, 76)]).astype(F))


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def remap_prim(prim, remap):
    """prim indices of a mesh with strays -> those of the clean mesh (the miss marker kept; a stray maps to 0xFFFFFFFE, which no clean
    result holds)"""
    prim = np.asarray(prim, np.uint32)
    hit = prim != rx.MISS
    out = prim.copy()
    m = np.asarray(remap)[prim[hit].astype(np.int64)]
    out[hit] = np.where(m >= 0, m, 0xFFFFFFFE).astype(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def oracle_counts(name, sat, k):
    """(setVoxel calls, occupied voxels, dims) of the CPU oracle on scaled(name, k)"""
    s = scaled(name, k)
    w, calls, gi = oracle.build_bool(s.v, s.t, s.vs, threads=0, sat=sat)
    return int(calls), int(np.unpackbits(w.view(np.uint8)).sum()), gi["dim"]


# ---- OBJ / MTL texts ----------------------------------------------------------------------------------------------------------------------
NUMERALS = ("1e999", "-1e999", "1e-999", "-1e-999", "1e300", "-1e300", "nan", "-inf", "+1.5", ".5e+1")


def numeral_f32(s):
    """Python's own reading of the numeral, rounded to float32 (beyond float32's range: +-Inf)"""
    with np.errstate(over="ignore"):
        return F(float(s))


def obj_texts():
    """-> (obj text, mtl text, expected vertices float32[V, 3], expected (Kd float32[M, 3], Ns float32[M])).  Every numeral stands as the
    first, middle and last component of a `v` line, directly behind a line of three other values, so that a reader which reuses a stale
    number shows it.  The MTL (scene.mtl beside the OBJ) puts the same numerals into Kd and Ns."""
    lines, verts = ["mtllib scene.mtl"], []
    n = 0
    for s in NUMERALS:
        for pos in range(3):
            n += 1
            before = [F(n + 0.25), F(-n - 0.5), F(2 * n + 0.125)]
            other = [F(100 + n), F(200 + n), F(300 + n)]
            lines.append("v %.9g %.9g %.9g" % tuple(before))
            verts.append(before)
            row = ["%.9g" % x for x in other]
            row[pos] = s
            lines.append("v " + " ".join(row))
            exp = list(other)
            exp[pos] = numeral_f32(s)
            verts.append(exp)
    lines += ["usemtl m0", "f 1 2 3"]
    mtl, kd, ns = [], [], []
    for i, s in enumerate(NUMERALS):
        row = [F(0.125 * (i + 1)), F(0.25 + i), F(0.5 + 2 * i)]
        exp = list(row)
        exp[i % 3] = numeral_f32(s)
        txt = ["%.9g" % x for x in row]
        txt[i % 3] = s
        mtl += ["newmtl m%d" % i, "Ns %.9g" % F(7 + i), "Kd " + " ".join(txt), "Ks 0.5 0.25 %.9g" % F(i + 3), "Ns " + s]
        kd.append(exp)
        ns.append(numeral_f32(s))
    return "\n".join(lines) + "\n", "\n".join(mtl) + "\n", np.array(verts, F), (np.array(kd, F), np.array(ns, F))


def same_f32(a, b):
    """equal as float32 values with NaN equal to NaN of either sign and -0 distinct from +0"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))
