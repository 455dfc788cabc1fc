"""What tests/test_gpu_walk_blocks32.py and tests/test_gpu_walk_siblings.py share: hand-built grids in the walk's permuted coordinates (the
Scene of tests/test_gpu_walk_early_finish.py), put through every first-hit query form under the four switch pairs, and through trace_multi
against tests/multihit_ref.py."""
import numpy as np

import multihit_ref as mr
import ray_extremes as rx
import test_gpu_walk_early_finish as ef

F = np.float32
MISS = ef.MISS
ORIENTATIONS = ef.ORIENTATIONS
ENVS = ef.ENVS
Scene = ef.Scene
same_bits = ef.same_bits
K_MULTI = 4
BIG = 1_064_960   # launch_walk: from this many rays on a batch takes the kernel that visits sibling bricks in travel order and prunes them


def through(cell, d, back):
    """a ray through the centre of `cell` along d, from `back` units of d in front of it (all in cell units, (u, v, w))"""
    c = np.array(cell, np.float64) + 0.5
    d = np.array(d, np.float64)
    return c - back * d, d


def at_and_below(sc):
    """a per-ray tmax: the reference's hit time for every other ray (the hit is still accepted), the float below it for the rest (it is not)"""
    return np.where(np.arange(len(sc.rays)) % 2 == 0, sc.ref_t, np.nextafter(sc.ref_t, F(0))).astype(F)


def scene(p, s, dims, vs=1.0, org=0.0):
    """a Scene whose constructions are written per travel direction (no mirror: a cell index means the same cell for both directions)"""
    return Scene(p, s, dims, vs=vs, org=org, mirror=False)


def kernel_tol(sc, rays=None):
    """walk_setup's position tolerance per ray"""
    r = sc.rays if rays is None else rays
    hi = np.array(sc.dim, F) * sc.vs + sc.org
    corner = max(abs(float(sc.org)), float(np.abs(hi).max()))
    return (np.maximum(np.abs(r[:, :3]).max(axis=1), F(corner)) * F(rx.TOL_FACTOR)).astype(F)


def check(gpu, sc, shadow=False, multi=True, tmax_per_ray=None, envs=ENVS, big=False):
    """the grid by hand; t and prim bit for bit through trace, trace_ex (t) and trace_ex (t, prim, normal) under the four switch pairs;
    any_hit; a per-ray tmax; trace_multi (k_multihit reads the same block level) against multihit_ref.  big: the rays again as a batch
    of BIG (repeated: what a ray returns does not depend on where in the batch it stands), the size from which the launch takes its
    other kernel -- the only one that orders and prunes sibling bricks -- under the four switch pairs through trace, trace_ex (t), any_hit
    and, where given, the per-ray tmax with its any_hit form."""
    X, Y, Z = sc.dim
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, Z, sc.vs, (float(sc.org),) * 3)
    try:
        for i in sc.order.tolist():
            g.set_voxel(i % X, (i // X) % Y, i // (X * Y))
        assert np.array_equal(g.bitmask(), sc.words)
        nhit = int((sc.ref_t > 0).sum())
        times = mr.hit_times(sc.oa, sc.rays) if (multi or tmax_per_ray is not None) and len(sc.oa) else None
        for lds, don in envs:
            what = (sc.p, sc.s, lds, don)
            with ef.env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=don):
                t, p, nh = g.trace(sc.rays, tmax=sc.tmax)
                assert same_bits(t, sc.ref_t) and np.array_equal(p, sc.ref_p) and nh == nhit, what
                k = g.trace_ex(sc.rays, tmax=sc.tmax, want=("t",))
                assert same_bits(k["t"], sc.ref_t), what
                k = g.trace_ex(sc.rays, tmax=sc.tmax, want=("t", "prim", "normal"))
                assert same_bits(k["t"], sc.ref_t) and np.array_equal(k["prim"], sc.ref_p), what
                if shadow:
                    sh = g.trace_ex(sc.rays, tmax=sc.tmax, any_hit=True, want=("shadowed",))["shadowed"]
                    assert np.array_equal(sh != 0, sc.ref_t > 0), what
                if tmax_per_ray is not None and times is not None:
                    rt, rp = rx.grid_closest_per_ray(times, 0.001, tmax_per_ray)
                    k = g.trace_ex(sc.rays, tmax_per_ray=tmax_per_ray, want=("t", "prim"))
                    assert same_bits(k["t"], rt) and np.array_equal(k["prim"], rp), what
                    sh = g.trace_ex(sc.rays, tmax_per_ray=tmax_per_ray, any_hit=True, want=("shadowed",))["shadowed"]
                    assert np.array_equal(sh != 0, rt > 0), what
        if big:
            idx = np.arange(BIG) % len(sc.rays)
            rays, rt, rp = np.ascontiguousarray(sc.rays[idx]), sc.ref_t[idx], sc.ref_p[idx]
            if tmax_per_ray is not None and times is not None:
                qt, qp = rx.grid_closest_per_ray(times, 0.001, tmax_per_ray)
                tpr_big, qt, qp = np.ascontiguousarray(np.asarray(tmax_per_ray, F)[idx]), qt[idx], qp[idx]
            for lds, don in envs:
                what = ("big", sc.p, sc.s, lds, don)
                with ef.env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=don):
                    t, p, nh = g.trace(rays, tmax=sc.tmax)
                    assert same_bits(t, rt) and np.array_equal(p, rp) and nh == int((rt > 0).sum()), what
                    k = g.trace_ex(rays, tmax=sc.tmax, want=("t",))
                    assert same_bits(k["t"], rt), what
                    if shadow:
                        sh = g.trace_ex(rays, tmax=sc.tmax, any_hit=True, want=("shadowed",))["shadowed"]
                        assert np.array_equal(sh != 0, rt > 0), what
                    if tmax_per_ray is not None and times is not None:
                        k = g.trace_ex(rays, tmax_per_ray=tpr_big, want=("t", "prim"))
                        assert same_bits(k["t"], qt) and np.array_equal(k["prim"], qp), what
                        sh = g.trace_ex(rays, tmax_per_ray=tpr_big, any_hit=True, want=("shadowed",))["shadowed"]
                        assert np.array_equal(sh != 0, qt > 0), what
        if multi and times is not None:
            rt, rp, rc = mr.select(times, K_MULTI, tmax=sc.tmax)
            got = g.trace_multi(sc.rays, max_hits=K_MULTI, tmax=sc.tmax)
            assert same_bits(got["t"], rt) and np.array_equal(got["prim"], rp) and np.array_equal(got["count"], rc), (sc.p, sc.s)
    finally:
        g.free()
