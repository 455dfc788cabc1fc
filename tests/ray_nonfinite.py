"""Non-finite rays: a ray with NaN, +Inf or -Inf in any of its six components is a miss on every ray query (include/voxhip.h, "Non-finite
rays").  Poisoned copies of hitting rays, batches that mix them with finite rays, and the expected outputs: the rule
for the poisoned rays, the unchanged brute-force references of tests/ray_extremes.py for the finite ones.  A helper for
tests/test_ray_nonfinite_cpu.py and tests/test_gpu_ray_nonfinite.py, not a test itself.

The finite rays of every scene are its "scaled" family at k = 0 (the suite's ordinary rays), whose references over [0, +inf] the ray-extremes
modules compute too: one copy per process, shared and left unchanged."""
import functools
import struct

import numpy as np

import ray_extremes as rx

F = np.float32
U = np.uint32
MISS = rx.MISS
POOL = ("scaled", 0)                  # the family the finite rays come from
OPEN = (0.0, np.inf)                  # the interval of every reference here
K = rx.K_MULTI
B = 64                                # base rays per scene
SCENES = (("grid", "rotcube"), ("grid", "wide"), ("bvh", "floor"), ("bvh", "adversarial"), ("tlas", "tlas"))

NAN, PINF, NINF = F(np.nan), F(np.inf), F(-np.inf)
VALUES = {"nan": NAN, "+inf": PINF, "-inf": NINF}
# NaNs with another payload, a set sign bit, and a signalling one (quiet bit clear, payload 1)
PATTERNS = {"0x7FC00001": 0x7FC00001, "0xFFC00000": 0xFFC00000, "0x7F800001": 0x7F800001}
COMP = ("ox", "oy", "oz", "dx", "dy", "dz")


def _bits(u):
    return np.array([u], U).view(F)[0]


def nonfinite(rays):
    """the rule's own predicate: any component NaN or +-Inf"""
    return ~np.isfinite(np.asarray(rays, F).reshape(-1, 6)).all(axis=1)


# ---- base rays and their poisoned copies -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(kind, name):
    return rx.family(kind, name, POOL)


@functools.lru_cache(maxsize=None)
def pool_closest(kind, name):
    """closest hit of every pool ray over [0, +inf] by the scene's unmodified brute force"""
    return rx.reference(kind, name, POOL, "closest", *OPEN)


@functools.lru_cache(maxsize=None)
def base_index(kind, name):
    """B pool rays that hit under [0, +inf], evenly spread over the hitting ones"""
    hits = np.flatnonzero(pool_closest(kind, name)["t"] > 0)
    return hits[np.linspace(0, len(hits) - 1, B).astype(int)]


def base(kind, name):
    return pool(kind, name)[base_index(kind, name)]


def poison_one(ray, j):
    """the poisoned copies of one base ray (the j-th of its scene: j picks the component where a copy poisons just one) -> [(label, ray)]"""
    out = []

    def add(label, **comp):
        r = ray.copy()
        for c, v in comp.items():
            r[COMP.index(c)] = v
        out.append((label, r))

    for c in COMP:                                               # every component x every value
        for vn, v in VALUES.items():
            add("%s %s" % (vn, "origin" if c[0] == "o" else "direction"), **{c: v})
    a = "xyz"[j % 3]
    for pn, p in PATTERNS.items():                               # NaN payloads, one direction and one origin component
        add("nan %s direction" % pn, **{"d" + a: _bits(p)})
        add("nan %s origin" % pn, **{"o" + "xyz"[(j + 1) % 3]: _bits(p)})
    add("nan two", **{"o" + a: NAN, "d" + "xyz"[(j + 1) % 3]: NAN})
    add("nan all six", **{c: NAN for c in COMP})
    for ax in "xyz":                                             # 0 * inf: the axis drops out of the brute force's slab test
        for so, sd in ((PINF, PINF), (PINF, NINF), (NINF, PINF), (NINF, NINF)):
            add("dropped axis (o, d = +-inf)", **{"o" + ax: so, "d" + ax: sd})
    add("nan origin on a zero-direction axis", **{"o" + a: NAN, "d" + a: F(0)})
    add("nan origin on a zero-direction axis", **{"o" + a: NAN, "d" + a: F(-0.0)})
    return out


@functools.lru_cache(maxsize=None)
def poisoned(kind, name):
    """-> (labels [P], rays [P, 6]): every poisoned copy of every base ray, base-major"""
    labels, rays = [], []
    for j, ray in enumerate(base(kind, name)):
        for label, r in poison_one(ray, j):
            labels.append(label)
            rays.append(r)
    rays = np.ascontiguousarray(np.stack(rays), F)
    assert nonfinite(rays).all()
    return tuple(labels), rx._frozen(rays)


LABELS = tuple(sorted({l for l, _ in poison_one(np.ones(6, F), 0)}))


# ---- where the rule departs from the unmodified brute force ----------------------------------------------------------------------------------
# (structure, label) pairs on which the unmodified reference reports a HIT for at least one poisoned copy: the answers the rule changes.
# Found by tests/test_ray_nonfinite_cpu.py::test_departures, which asserts this very set; DESIGN.md section 6n carries the list.
# The voxel brute force (hitAabb with NaN-dropping min / max, which is also the octree's reference) loses the poisoned axis and tests the
# other two; Moeller-Trumbore (mesh_ref, instance_ref) carries a NaN or an infinity into u, v or t of every triangle and accepts nothing.
_VOXEL_DEPARTURES = ("nan origin", "nan direction", "nan 0x7FC00001 origin", "nan 0x7FC00001 direction", "nan 0xFFC00000 origin",
                     "nan 0xFFC00000 direction", "nan 0x7F800001 origin", "nan 0x7F800001 direction", "nan two", "dropped axis (o, d = +-inf)",
                     "nan origin on a zero-direction axis")
DEPARTURES = frozenset(("grid", l) for l in _VOXEL_DEPARTURES)


def reference_hits(kind, name, rays):
    """hit flags of the scene's UNMODIFIED closest-hit reference over [0, +inf] on arbitrary (non-finite) rays"""
    with np.errstate(all="ignore"):
        return rx.ref_closest(kind, rx.scene_of(kind, name), rays, *OPEN)["t"] > 0


# ---- batches -----------------------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 63, 64, 65, 257, "runs", "all")


@functools.lru_cache(maxsize=None)
def batch(kind, name, which, multi=False):
    """-> (src, rays): src[i] >= 0: finite ray src[i] of the pool; src[i] = -1: a poisoned ray.  multi: the pool is the one the multi-hit
    reference runs on (rx.multi_rays: the same rays, but on the wide grid rx.N_MULTI_WIDE of them).
    which = a size (1, 63, 64, 65, 257: a seeded mix, about a third poisoned, the single ray poisoned); "runs": 4000 rays -- isolated poisoned
    rays, poisoned first and last lanes of a wave, one whole poisoned wave, and 300 consecutive poisoned rays that cover rays 2048 .. 2303,
    which is one whole dynamic chunk of k_walk at its largest; "all": 1000 poisoned rays."""
    p = rx.multi_rays(kind, name, POOL) if multi else pool(kind, name)
    npool = len(p)
    _, bad = poisoned(kind, name)
    rng = np.random.default_rng(1000 + BATCHES.index(which))
    if which == "all":
        n, mask = 1000, np.ones(1000, bool)
    elif which == "runs":
        n = 4000
        mask = np.zeros(n, bool)
        mask[rng.choice(n, 40, replace=False)] = True            # isolated
        mask[[0, 63, 128, 191 + 64, n - 1]] = True               # first lanes, last lanes, the batch's last ray
        mask[1024:1088] = True                                   # one whole wave
        mask[2030:2330] = True                                   # 300 in a row, rays 2048 .. 2303 among them
    else:
        n = which
        mask = rng.random(n) < 0.35
        mask[0] = True
    src = np.where(mask, -1, rng.integers(0, npool, n))
    rays = p[np.maximum(src, 0)].copy()
    rays[mask] = bad[rng.integers(0, len(bad), int(mask.sum()))]
    assert np.array_equal(nonfinite(rays), mask)
    return rx._frozen(src), rx._frozen(np.ascontiguousarray(rays, F))


# ---- expected values: the rule on the poisoned rays, the reference on the finite ones -----------------------------------------------------------
RULE = {"t": F(-1), "prim": MISS, "instance": MISS, "bary": F(0), "normal": F(0), "shadowed": np.uint8(0), "count": U(0)}


def masked(src, ref):
    """ref: dict of per-pool-ray reference outputs (or one array) -> the same for the batch `src`"""
    if not isinstance(ref, dict):
        return masked(src, {"x": ref})["x"]
    out = {}
    dead = src < 0
    for f, v in ref.items():
        v = np.asarray(v)
        g = v[np.maximum(src, 0)].copy()
        g[dead] = RULE[f]
        out[f] = g
    return out


def all_miss(n, fields, k=None):
    """the rule's outputs for n rays (k: multi-hit lists of k slots)"""
    shape = {"bary": (2,), "normal": (3,)}
    out = {}
    for f in fields:
        s = (n,) + (() if k is None or f == "count" else (k,)) + shape.get(f, ())
        out[f] = np.full(s, RULE[f], np.asarray(RULE[f]).dtype)
    return out


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------------
W = H = 8


def cameras():
    """-> {name: (view_inverse, proj_inverse, W, H)}: a NaN translation in view_inverse (every origin NaN); an all-zero proj_inverse (every
    direction NaN through 1 / sqrt(0)); and, for comparison, a finite camera that looks away from the scene (every pixel a plain miss)"""
    import vx_scenes
    vi, pi = vx_scenes.camera_matrices(aspect=1.0)
    nan_t = vi.copy()
    nan_t[13] = NAN
    away_vi, away_pi = vx_scenes.camera_matrices(eye=(6.16636, 2.42256, -3.15471), ctr=(60.0, 30.0, -30.0), aspect=1.0)
    return {"nan translation": (nan_t, pi, W, H), "zero projection": (vi, np.zeros(16, F), W, H), "away": (away_vi, away_pi, W, H)}


# ---- the CPU walker's stand-alone check ----------------------------------------------------------------------------------------------------------
def write_walk_case(path):
    """the input of oracle/walk_check.c: the rotcube grid, its pool rays with the walker's own results on them (which
    tests/test_ray_extremes_cpu.py proves equal to the brute force), then every poisoned copy"""
    import oracle
    sc = rx.grid_scene("rotcube")
    fin = pool("grid", "rotcube")
    _, bad = poisoned("grid", "rotcube")
    w = np.ascontiguousarray(sc.ow, U)
    dim = np.array(sc.gi["dim"], np.uint64)
    org = np.ascontiguousarray(sc.gi["bmin"], F)
    t = np.full(len(fin), -1.0, F)
    idx = np.full(len(fin), 0xFFFFFFFFFFFFFFFF, np.uint64)
    h = oracle.lib().vxo_walk_create(oracle._u32(w), oracle._u64(dim), F(sc.vs), oracle._f(org))
    try:
        oracle.lib().vxo_walk_trace(h, oracle._f(fin), len(fin), F(0.001), F(10000.0), 1, oracle._f(t), oracle._u64(idx), None)
    finally:
        oracle.lib().vxo_walk_free(h)
    rays = np.ascontiguousarray(np.concatenate([fin, bad]), F)
    with open(path, "wb") as fh:
        fh.write(dim.tobytes() + struct.pack("<f", float(sc.vs)) + org.tobytes() + struct.pack("<3Q", len(w), len(rays), len(fin)))
        fh.write(w.tobytes() + rays.tobytes() + t.tobytes() + idx.tobytes())
    return len(fin), len(bad)
