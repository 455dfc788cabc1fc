"""The ray regimes of tests/ray_extremes.py on the references alone, before any GPU sees them: every family still hits (no family
degenerates into all-miss), the far origins reach the regimes of k_walk they are meant for, the grid-walking checker equals the brute
force on every grid family and interval, and the exact relations that need no reference -- d * 2^k scales every t by 2^-k and nothing
else, the interval is closed at both ends -- hold in every reference."""
import numpy as np
import pytest

import oracle
import ray_extremes as rx

F = np.float32
SCENES = [("grid", n) for n in rx.GRID_SCENES] + [("bvh", n) for n in rx.BVH_SCENES] + [("tlas", "tlas")]
WIDE_OPEN = (0.0, np.inf)


def rate(t):
    return float((np.asarray(t) > 0).mean())


def multi_rate(m):
    return float((m["count"] > 0).mean())


@pytest.mark.parametrize("kind,name", SCENES)
def test_hit_rate_floors(kind, name):
    """families 1, 3 and 4 hit at least HIT_FLOOR of their rays in every reference; family 2 hits what its unscaled rays hit"""
    def rates(fam, *interval):
        out = [rate(rx.reference(kind, name, fam, "closest", *interval)["t"]), float(rx.reference(kind, name, fam, "any", *interval).mean())]
        if fam[0] in ("far", "scaled"):
            out.append(float((rx.reference(kind, name, fam, "multi", *interval)["count"] > 0).mean()))
        return out

    for D, shape in rx.far_keys(kind, name):
        assert min(rates(("far", D, shape), *WIDE_OPEN)) >= rx.HIT_FLOOR, (D, shape)
    unscaled = min(rates(("scaled", 0), *WIDE_OPEN))
    assert unscaled >= rx.HIT_FLOOR
    for k in rx.K_SCALES:
        assert min(rates(("scaled", k), *WIDE_OPEN)) >= unscaled, k
    for which in ("finite", "infinite"):
        assert min(rates(("subnormal", which))) >= rx.HIT_FLOOR, which
    assert rate(rx.t_star(kind, name)["t"]) >= rx.HIT_FLOOR


@pytest.mark.parametrize("name", rx.GRID_SCENES)
def test_far_origins_reach_the_window_regime(name):
    """walk_setup's tol against the voxel size: D >= 1e6 puts EVERY ray in the regime where tol reaches a brick (8 voxels: the per-slab
    rectangle outgrows one 16-cell window), D = 1e3 leaves every ray in the ordinary one (tol below a voxel).  The wide grid's own
    extent is 10^5 voxels: D = 1e3 and above are in the window regime already and D = 1e2 is halfway there."""
    sc = rx.grid_scene(name)
    seen = set()
    for D, shape in rx.far_keys("grid", name):
        tol = rx.walk_tol(sc, rx.far_family("grid", name, D, shape))
        if D >= 1e6 or (name == "wide" and D >= 1e3):
            assert (tol >= F(8) * sc.vs).all(), (D, shape, float(tol.min() / sc.vs))
            seen.add("window")
        elif name == "wide":
            assert (tol >= F(4) * sc.vs).all(), (D, shape, float(tol.min() / sc.vs))   # rectangles of 8 cells and more across
        elif D == 1e3:
            assert (tol < sc.vs).all(), (D, shape, float(tol.max() / sc.vs))
            seen.add("ordinary")
    assert "window" in seen and (name == "wide" or "ordinary" in seen)
    assert (rx.walk_tol(sc, rx.base_rays("grid", name)) < sc.vs).all()


def grid_intervals(name):
    """every (rays, tmin, tmax) the grid tests of the GPU file trace with a scalar interval"""
    for D, shape in rx.far_keys("grid", name):
        yield "far %g %s" % (D, shape), rx.far_family("grid", name, D, shape), 0.0, np.inf
    for k in rx.K_SCALES:
        yield "scaled %d open" % k, rx.scaled_family("grid", name, k), 0.0, np.inf
        yield "scaled %d default" % k, rx.scaled_family("grid", name, k), 0.001, 10000.0
    for which in ("finite", "infinite"):
        yield "subnormal " + which, rx.subnormal_family("grid", name, which), 0.001, 10000.0
    rays = rx.interval_rays("grid", name)
    for tmin, tmax in rx.SCALAR_INTERVALS + rx.EMPTY_INTERVALS:
        yield "interval [%g, %g]" % (tmin, tmax), rays, tmin, tmax
    batch, picks = rx.exact_cases("grid", name)
    for j, ts in picks:
        for label, (tmin, tmax) in rx.exact_intervals(ts).items():
            yield "exact %s ray %d" % (label, j), batch, tmin, tmax


@pytest.mark.parametrize("name", rx.GRID_SCENES)
def test_grid_walk_equals_brute_force(name):
    """oracle.trace_walk, the checker of the large GPU tests, returns the brute-force minimum bit for bit on every grid family"""
    sc = rx.grid_scene(name)
    for what, rays, tmin, tmax in grid_intervals(name):
        ot, op = oracle.trace_brute(sc.oa, rays, tmin, tmax)
        wt, wp = oracle.trace_walk(sc.ow, sc.gi, sc.vs, rays, tmin, tmax)
        assert rx.same_bits(wt, ot) and np.array_equal(wp, op), (what, rx.first_difference({"t": wt, "prim": wp}, {"t": ot, "prim": op}, rays))
        # the shadow query over the same interval: shadowed iff a closest hit exists
        assert np.array_equal(oracle.trace_any_brute(sc.oa, rays, tmin, tmax).astype(bool), ot > 0), what


def assert_scaled(ref0, refk, k, what, safe):
    """refk == ref0 with every hit time times 2^-k: prim, bary, instance and count bit-identical on the rays where the scaling is exact"""
    for f in ref0:
        want = rx.scaled_t(ref0[f], k) if f == "t" else ref0[f]
        assert rx.same_bits(refk[f][safe], want[safe]), (what, f, k)


@pytest.mark.parametrize("kind,name", SCENES)
def test_scaling_relation(kind, name):
    """d * 2^k over [0, +inf]: every t times 2^-k exactly, everything else unchanged -- in the closest-hit and the multi-hit references;
    over the default interval the scaled-down directions put every t beyond tmax and the scaled-up ones below tmin"""
    c0 = rx.reference(kind, name, ("scaled", 0), "closest", *WIDE_OPEN)
    m0 = rx.reference(kind, name, ("scaled", 0), "multi", *WIDE_OPEN)
    for k in rx.K_SCALES:
        safe = rx.scale_safe(kind, name, k)
        assert safe.mean() >= 0.9 and (safe.all() or (kind != "grid" and k < 0)), (k, safe.mean())
        assert_scaled(c0, rx.reference(kind, name, ("scaled", k), "closest", *WIDE_OPEN), k, "closest", safe)
        ms = safe[:len(m0["count"])] if safe.all() else safe          # (the wide grid's multi-hit subset: a grid, every ray safe)
        assert_scaled(m0, rx.reference(kind, name, ("scaled", k), "multi", *WIDE_OPEN), k, "multi", ms)
        if k != 0:
            assert not (rx.reference(kind, name, ("scaled", k), "closest")["t"] > 0).any(), k
            assert not rx.reference(kind, name, ("scaled", k), "any").any(), k


@pytest.mark.parametrize("kind,name", SCENES)
def test_interval_identities(kind, name):
    sc = rx.scene_of(kind, name)
    rays = rx.interval_rays(kind, name)
    star = rx.t_star(kind, name)
    hit = star["t"] > 0
    # tmin <= 0 rejects nothing that t > 0 admits; every finite t is within FLT_MAX
    for tmin, tmax in rx.SCALAR_INTERVALS:
        got = rx.ref_closest(kind, sc, rays, tmin, tmax)
        assert rx.first_difference(got, star, rays) is None, (tmin, tmax)
        assert np.array_equal(rx.ref_any(kind, sc, rays, tmin, tmax).astype(bool), hit)
    for tmin, tmax in rx.EMPTY_INTERVALS:
        assert not (rx.ref_closest(kind, sc, rays, tmin, tmax)["t"] > 0).any() and not rx.ref_any(kind, sc, rays, tmin, tmax).any()
        m = rx.ref_multi(kind, sc, rays[:200 if (kind, name) != ("grid", "wide") else rx.N_MULTI_WIDE], tmin, tmax)
        assert not m["count"].any() and (m["t"] == -1).all()
    # the interval is closed at both ends
    batch, picks = rx.exact_cases(kind, name)
    assert len(picks) == 6
    for j, ts in picks:
        iv = rx.exact_intervals(ts)
        at = rx.ref_closest(kind, sc, batch, *iv["at"])
        assert at["t"][j] == ts and at["prim"][j] == star["prim"][j] and rx.ref_any(kind, sc, batch, *iv["at"])[j] == 1
        assert (at["t"][at["t"] > 0] == ts).all()
        above = rx.ref_closest(kind, sc, batch, *iv["above"])["t"][j]
        assert above == -1 or above > ts
        assert rx.ref_closest(kind, sc, batch, *iv["below"])["t"][j] == -1 and rx.ref_any(kind, sc, batch, *iv["below"])[j] == 0
    # per-ray tmax
    cases = rx.per_ray_tmax_cases(star["t"])
    for label, tm in cases.items():
        got = rx.ref_closest(kind, sc, rays, 0.0, 1.0, tmax_per_ray=tm)          # the scalar tmax is replaced, whatever it is
        sh = rx.ref_any(kind, sc, rays, 0.0, 1.0, tmax_per_ray=tm)
        with np.errstate(invalid="ignore"):
            keep = hit & (star["t"] <= tm)
        assert np.array_equal(got["t"] > 0, keep) and np.array_equal(sh.astype(bool), keep), label
        assert rx.same_bits(got["t"][keep], star["t"][keep]) and np.array_equal(got["prim"][keep], star["prim"][keep]), label
        if label in ("zero", "minus_one", "below_t_star"):
            assert not keep.any()
        if label in ("t_star", "inf"):
            assert np.array_equal(keep, hit)
    assert 0 < (rx.ref_closest(kind, sc, rays, 0.0, 1.0, tmax_per_ray=cases["mixed"])["t"] > 0).sum() < hit.sum()


@pytest.mark.parametrize("name", ["rotcube", "adversarial"])
def test_grid_per_ray_tmax_reference(name):
    """ref_closest derives the grid's per-ray-tmax closest hit from the brute force over [tmin, +inf]; the definition (the minimum over the
    boxes accepted under each ray's own tmax) gives the same"""
    import multihit_ref as mr
    sc = rx.grid_scene(name)
    rays = rx.interval_rays("grid", name)
    times = mr.hit_times(sc.oa, rays)
    for label, tm in rx.per_ray_tmax_cases(rx.t_star("grid", name)["t"]).items():
        t, p = rx.grid_closest_per_ray(times, 0.0, tm)
        got = rx.ref_closest("grid", sc, rays, 0.0, 1.0, tmax_per_ray=tm)
        assert rx.same_bits(got["t"], t) and np.array_equal(got["prim"], p), label
    rng = np.random.default_rng(5)
    tm = rng.uniform(0.0, 12.0, len(rays)).astype(F)
    t, p = rx.grid_closest_per_ray(times, 0.001, tm)
    got = rx.ref_closest("grid", sc, rays, 0.001, 1.0, tmax_per_ray=tm)
    assert rx.same_bits(got["t"], t) and np.array_equal(got["prim"], p) and 0 < (t > 0).sum() < len(t)
