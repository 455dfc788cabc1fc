"""GPU tests of every ray tracer in the regimes of tests/ray_extremes.py: origins 10^3 .. 10^7 scene diagonals away (k_walk's window path, the
relative widening of box_enter, k_octree_trace's pruning, k_tlas_trace moving a far ray into object space), directions scaled by 2^-100 ..
2^100, subnormal direction components on both sides of the finite-reciprocal boundary, and the edges of the ray interval.  Every output is
bit-equal to the float32 brute force of the same pinned formula over all rays of a family; the scaling relation is also asserted on the GPU
outputs alone.  tests/test_ray_extremes_cpu.py checks the families and the references themselves."""
import numpy as np
import pytest

import instance_ref
import mesh_ref
import oracle
import ray_extremes as rx
from test_gpu_configs import env

pytestmark = pytest.mark.gpu

F = np.float32
OPEN = (0.0, np.inf)
DEFAULT = (0.001, 10000.0)
LEAVES = (1, 0)                      # BVH leaf sizes: one triangle, and the library default
SMALL_GRIDS = ("rotcube", "adversarial")
_handles = {}


def handle(vx, kind, name, arg=None):
    """one device structure per (kind, scene, argument) for the whole module"""
    key = (kind, name, arg)
    if key not in _handles:
        sc = rx.scene_of("grid" if kind == "octree" else kind, name)
        if kind == "grid":
            h = vx.Grid.voxelize(vx.Mesh.from_arrays(sc.v, sc.t), sc.vs)
        elif kind == "octree":
            h = vx.Octree(vx.Mesh.from_arrays(sc.v, sc.t), sc.vs)
        elif kind == "bvh":
            h = vx.Mesh.from_arrays(sc.v, sc.t).bvh(max_leaf=arg)
        else:
            blas = [vx.Bvh(vx.Mesh.from_arrays(v, t), max_leaf=arg) for v, t in sc.meshes]
            h = (vx.Tlas(blas, sc.inst), blas)
        _handles[key] = h
    return _handles[key]


def same(got, ref, rays, what):
    diff = rx.first_difference(got, ref, rays)
    assert diff is None, "%s: %s" % (what, diff)


# ---- the references of one (family, interval), per structure --------------------------------------------------------------------------------
class Ref:
    """closest / any / multi of a structure's reference on a family of tests/ray_extremes.py"""

    def __init__(self, kind, name, boxes=None):
        self.kind, self.name, self.boxes = kind, name, boxes
        self.sc = rx.scene_of(kind, name)
        self.has_multi = boxes is None                  # the octree has no multi-hit query

    def closest(self, fam, tmin, tmax, tmax_per_ray=None):
        rays = rx.family(self.kind, self.name, fam)
        wide = self.kind == "grid" and self.name == "wide" and self.boxes is None
        if wide and tmax_per_ray is not None:
            # as rx.ref_closest derives it: the closest hit of [tmin, +inf] where it lies at or below the ray's own tmax
            out = self.closest(fam, tmin, np.inf)
            keep = (out["t"] > 0) & (out["t"] <= np.asarray(tmax_per_ray, F))
            return {"t": np.where(keep, out["t"], F(-1)).astype(F), "prim": np.where(keep, out["prim"], rx.MISS).astype(np.uint32)}
        if wide:
            # 860 430 boxes: the grid-walking checker, which the CPU test proves equal to the brute force on these very families
            t, p = oracle.trace_walk(self.sc.ow, self.sc.gi, self.sc.vs, rays, tmin, tmax)
            out = {"t": t, "prim": p}
        elif self.boxes is None and tmax_per_ray is None:
            out = dict(rx.reference(self.kind, self.name, fam, "closest", tmin, tmax))
        else:
            out = rx.ref_closest(self.kind, self.sc, rays, tmin, tmax, tmax_per_ray, boxes=self.boxes)
        if self.kind == "grid":
            out["normal"] = oracle.cube_normals(self.sc.oa if self.boxes is None else self.boxes, out["prim"], rays, out["t"])
        return out

    def any(self, fam, tmin, tmax, tmax_per_ray=None, closest_t=None):
        if self.kind == "grid" and self.name == "wide" and self.boxes is None:
            return (closest_t > 0).astype(np.uint8)          # same interval: shadowed iff a closest hit exists (the CPU test asserts it)
        if self.boxes is None and tmax_per_ray is None:
            return rx.reference(self.kind, self.name, fam, "any", tmin, tmax)
        return rx.ref_any(self.kind, self.sc, rx.family(self.kind, self.name, fam), tmin, tmax, tmax_per_ray, boxes=self.boxes)

    def multi(self, fam, tmin, tmax):
        return rx.reference(self.kind, self.name, fam, "multi", tmin, tmax)


WANT = {"grid": ("t", "prim", "normal"), "bvh": ("t", "prim", "bary", "normal"), "tlas": ("t", "instance", "prim", "bary", "normal")}
WANT_MULTI = {"grid": ("t", "prim", "count"), "bvh": ("t", "prim", "bary", "count"), "tlas": ("t", "instance", "prim", "bary", "count")}


def check_normals(ref, got, exp, rays, what):
    """grids: the cube-face normal, bit-equal; meshes: the unit geometric normal of the reported triangle to the suite's own tolerances"""
    sc = ref.sc
    if ref.kind == "grid":
        return same({"normal": got["normal"]}, {"normal": exp["normal"]}, rays, what + " normal")
    with np.errstate(all="ignore"):
        if ref.kind == "bvh":
            nrm, tol = mesh_ref.normals(sc.v, sc.t, got["prim"]), 1e-6
        else:
            nrm, tol = instance_ref.world_normals(sc.meshes, sc.inst, got["instance"], got["prim"]), 4e-6
    hit = got["t"] > 0
    unit = np.isfinite(nrm).all(axis=1)          # a point-sized or collinear triangle has no unit normal: 0 / 0 in the reference
    assert (unit & hit).sum() > 0.9 * hit.sum() or not hit.any(), what + " normal: too few hits on a triangle with a normal"
    assert np.abs(got["normal"][unit] - nrm[unit]).max() <= tol, what + " normal"


def check_family(tracer, ref, fam, tmin, tmax, what, full=True, multi=False, tmax_per_ray=None):
    """closest hit and shadow query (and K = 4 multi-hit) of `tracer` on a family against `ref`; -> the GPU's closest-hit outputs"""
    rays = rx.family(ref.kind, ref.name, fam)
    kw = dict(tmin=tmin, tmax=tmax, tmax_per_ray=tmax_per_ray)
    exp = ref.closest(fam, tmin, tmax, tmax_per_ray)
    want = WANT[ref.kind] if full else tuple(w for w in WANT[ref.kind] if w != "normal")
    got = tracer.trace_ex(rays, want=want, **kw)
    same(got, {k: v for k, v in exp.items() if k != "normal"}, rays, what + " closest")
    if full:
        check_normals(ref, got, exp, rays, what)
    sh = tracer.trace_ex(rays, any_hit=True, want=("shadowed",), **kw)["shadowed"]
    same({"shadowed": sh}, {"shadowed": ref.any(fam, tmin, tmax, tmax_per_ray, closest_t=exp["t"])}, rays, what + " any_hit")
    if multi and ref.has_multi:
        mrays = rx.multi_rays(ref.kind, ref.name, fam)           # the family itself, but on the wide grid: rx.N_MULTI_WIDE rays of it
        gm = tracer.trace_multi(mrays, max_hits=rx.K_MULTI, tmin=tmin, tmax=tmax, want=WANT_MULTI[ref.kind])
        if (exp["t"] > 0).any():
            same(gm, ref.multi(fam, tmin, tmax), mrays, what + " multi")
        else:   # the closest-hit reference accepts nothing on any ray: the accepted set, which is the multi-hit query's too, is empty
            assert not gm["count"].any() and (gm["t"] == -1).all() and (gm["prim"] == rx.MISS).all(), what + " multi"
        got["multi"] = gm
    return got


def check_num_hits(tracer, ref, fam, tmin, tmax, what):
    """the plain entry point: t, prim and num_hits"""
    rays = rx.family(ref.kind, ref.name, fam)
    exp = ref.closest(fam, tmin, tmax)
    out = tracer.trace(rays, tmin, tmax)
    got = {"t": out[0], "instance": out[1], "prim": out[2]} if ref.kind == "tlas" else {"t": out[0], "prim": out[1]}
    same(got, {k: exp[k] for k in got}, rays, what + " trace")
    assert out[-1] == int((exp["t"] > 0).sum()), what + " num_hits"


def assert_metamorphic(outs, ref, what):
    """outs[k] = the GPU's outputs on d * 2^k over [0, +inf]: t * 2^-k, everything else bit-identical, on the rays where scaling is exact"""
    base = outs[0]
    rays = rx.family(ref.kind, ref.name, ("scaled", 0))
    for k, out in outs.items():
        for part, b, r in ((out, base, rays), (out.get("multi"), base.get("multi"), rx.multi_rays(ref.kind, ref.name, ("scaled", 0)))):
            if part is None:
                continue
            safe = rx.scale_safe(ref.kind, ref.name, k)
            if len(r) != len(safe):
                assert safe.all()                    # the wide grid's multi-hit subset: a grid, every ray scales exactly
                safe = safe[:len(r)]
            exp = {f: (rx.scaled_t(v, k) if f == "t" else v)[safe] for f, v in b.items() if f not in ("multi", "normal")}
            same({f: v[safe] for f, v in part.items() if f in exp}, exp, r[safe], "%s k=%d against k=0" % (what, k))


def run_far(tracer, ref, what):
    for D, shape in rx.far_keys(ref.kind, ref.name):
        fam = ("far", D, shape)
        label = "%s far D=%g %s" % (what, D, shape)
        check_family(tracer, ref, fam, *OPEN, label, multi=True)
        if hasattr(tracer, "trace"):
            check_num_hits(tracer, ref, fam, *OPEN, label)


def run_scaled(tracer, ref, what):
    outs = {}
    for k in rx.K_SCALES:
        fam = ("scaled", k)
        outs[k] = check_family(tracer, ref, fam, *OPEN, "%s scaled k=%d open" % (what, k), multi=True)
        got = check_family(tracer, ref, fam, *DEFAULT, "%s scaled k=%d default" % (what, k), multi=True)
        if k != 0:
            assert not (got["t"] > 0).any() and (got["prim"] == rx.MISS).all(), (what, k)    # every t beyond tmax, or below tmin
    assert_metamorphic(outs, ref, what)


def run_subnormal(tracer, ref, what):
    for which in ("finite", "infinite"):
        got = check_family(tracer, ref, ("subnormal", which), *DEFAULT, "%s subnormal %s" % (what, which), full=False)
        assert (got["t"] > 0).mean() >= rx.HIT_FLOOR


INTERVAL_PARTS = ("scalar", "empty", "exact", "per_ray")


def run_intervals(tracer, ref, what, parts=INTERVAL_PARTS):
    fam = ("interval",)
    star = ref.closest(fam, *OPEN)
    for tmin, tmax in rx.SCALAR_INTERVALS if "scalar" in parts else ():
        got = check_family(tracer, ref, fam, tmin, tmax, "%s [%g, %g]" % (what, tmin, tmax), full=False)
        assert rx.same_bits(got["t"], star["t"]) and np.array_equal(got["prim"], star["prim"])
        if hasattr(tracer, "trace"):
            check_num_hits(tracer, ref, fam, tmin, tmax, "%s [%g, %g]" % (what, tmin, tmax))
    for tmin, tmax in rx.EMPTY_INTERVALS if "empty" in parts else ():
        got = check_family(tracer, ref, fam, tmin, tmax, "%s [%g, %g]" % (what, tmin, tmax), full=False)
        assert (got["t"] == -1).all() and (got["prim"] == rx.MISS).all()
        if hasattr(tracer, "trace"):
            assert tracer.trace(rx.family(ref.kind, ref.name, fam), tmin, tmax)[-1] == 0                # num_hits
        if hasattr(tracer, "trace_multi"):
            m = tracer.trace_multi(rx.family(ref.kind, ref.name, fam), max_hits=rx.K_MULTI, tmin=tmin, tmax=tmax, want=("t", "count"))
            assert not m["count"].any() and (m["t"] == -1).all()
    _, picks = rx.exact_cases(ref.kind, ref.name, tstar=star["t"])       # t* of this structure's own boxes
    for j, ts in picks if "exact" in parts else ():
        iv = rx.exact_intervals(ts)
        got = check_family(tracer, ref, ("exact",), *iv["at"], "%s tmin = tmax = t* of ray %d" % (what, j), full=False)
        assert got["t"][j] == ts and got["prim"][j] == star["prim"][j]
        got = check_family(tracer, ref, ("exact",), *iv["above"], "%s tmin just above t* of ray %d" % (what, j), full=False)
        assert got["t"][j] == -1 or got["t"][j] > ts
        got = check_family(tracer, ref, ("exact",), *iv["below"], "%s tmax just below t* of ray %d" % (what, j), full=False)
        assert got["t"][j] == -1
    for label, tm in rx.per_ray_tmax_cases(star["t"]).items() if "per_ray" in parts else ():
        got = check_family(tracer, ref, fam, 0.0, 1.0, "%s per-ray tmax %s" % (what, label), full=False, tmax_per_ray=tm)
        if label in ("zero", "minus_one", "below_t_star"):
            assert (got["t"] == -1).all()
        if label in ("t_star", "inf"):
            assert rx.same_bits(got["t"], star["t"])


RUNS = {"far": run_far, "scaled": run_scaled, "subnormal": run_subnormal, "intervals": run_intervals}


# ---- voxel grids: k_walk and the multi-hit walk ----------------------------------------------------------------------------------------------
# (the far family of the 100 000 x 8 x 8 grid -- k_walk's WIDE variants, rectangles of up to 4770 bricks per slab, slow by design -- runs one
# origin distance per case below)
GRID_CASES = [(n, f) for n in rx.GRID_SCENES for f in RUNS if (n, f) != ("wide", "far")]


@pytest.mark.parametrize("name,family", GRID_CASES)
def test_grid(gpu, name, family):
    RUNS[family](handle(gpu, "grid", name), Ref("grid", name), "grid " + name)


@pytest.mark.parametrize("D,shape", rx.far_keys("grid", "wide"))
def test_grid_wide_far(gpu, D, shape):
    g, ref = handle(gpu, "grid", "wide"), Ref("grid", "wide")
    fam, label = ("far", D, shape), "grid wide far D=%g %s" % (D, shape)
    check_family(g, ref, fam, *OPEN, label, multi=True)
    check_num_hits(g, ref, fam, *OPEN, label)


# the 100 000 x 8 x 8 grid reads its mips from global memory whatever is asked: its one other path is the walk without work donation
FORCED = [(n, l, d) for n in SMALL_GRIDS for l, d in ((0, 1), (1, 0), (0, 0))] + [("wide", 0, 0)]


@pytest.mark.parametrize("name,lds,donate", FORCED)
def test_grid_far_origins_forced_paths(gpu, name, lds, donate):
    """family 1 once more with the mips read from global memory and / or without work donation"""
    g, ref = handle(gpu, "grid", name), Ref("grid", name)
    with env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=donate):
        for D, shape in rx.far_keys("grid", name):
            check_num_hits(g, ref, ("far", D, shape), *OPEN, "grid %s lds=%d donate=%d far D=%g %s" % (name, lds, donate, D, shape))


# ---- octree: k_octree_trace over the octree's own box list -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(RUNS))
@pytest.mark.parametrize("name", SMALL_GRIDS)
def test_octree(gpu, name, family):
    o = handle(gpu, "octree", name)
    RUNS[family](o, Ref("grid", name, boxes=o.aabbs()), "octree " + name)


@pytest.mark.parametrize("family", [f for f in RUNS if f != "intervals"] + ["intervals-" + p for p in INTERVAL_PARTS])
def test_octree_wide(gpu, family):
    """the 100 000 x 8 x 8 octree against the brute force over its 860 430 boxes (the interval family one part per case: every call
    is a pass over all boxes)"""
    o = handle(gpu, "octree", "wide")
    ref = Ref("grid", "wide", boxes=o.aabbs())
    if family.startswith("intervals-"):
        run_intervals(o, ref, "octree wide", parts=(family[len("intervals-"):],))
    else:
        RUNS[family](o, ref, "octree wide")


# ---- triangle BVH and instanced scene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(RUNS))
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", rx.BVH_SCENES)
def test_bvh(gpu, name, leaf, family):
    RUNS[family](handle(gpu, "bvh", name, leaf), Ref("bvh", name), "bvh %s max_leaf=%d" % (name, leaf))


@pytest.mark.parametrize("family", list(RUNS))
@pytest.mark.parametrize("leaf", LEAVES)
def test_tlas(gpu, leaf, family):
    RUNS[family](handle(gpu, "tlas", "tlas", leaf)[0], Ref("tlas", "tlas"), "tlas max_leaf=%d" % leaf)
