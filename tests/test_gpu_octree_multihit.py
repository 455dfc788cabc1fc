"""GPU tests of the multi-hit ray query on the octree (vx_octree_trace_multi*, Octree.trace_multi, k_octree_multihit): ordered hit lists and
hit counts are compared whole, bit for bit (t through its uint32 view), with the brute force over the octree's own de-duplicated AABB list
(tests/octree_multihit_ref.py, whose preconditions tests/test_octree_multihit_cpu.py proves on the CPU)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import multihit_ref as mr
import octree_multihit_ref as om
import ray_nonfinite as rn
import vx_scenes
from test_gpu_multihit import family_rays, same
from test_gpu_octree_trace import two_cluster_mesh, zero_component_rays
from test_gpu_parity import long_thin_mesh

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
KS = (1, 3, 8, 32)
# with KS: every compiled list size KC = 4, 8, 16, 32 exactly full (K = KC) and at its smallest K (5, 9, 17); at one leaf size
MORE_KS = (4, 5, 9, 16, 17)
LEAF_SIZES = (1, 16, 100)     # the direct node-array form (<= 64) and the level-by-level form (> 64)
ALL_SCENES = om.SCENES + (om.TIE,)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, vs):
    """mesh, one octree per leaf size, their common list, the rays and the matrix of reference hit times -- built once per scene and left
    unchanged"""
    import oracle
    import voxhip as gpu
    c = Case()
    c.v, c.t = om.mesh(name)
    c.vs = F(vs)
    c.mesh = gpu.Mesh.from_arrays(c.v, c.t)
    c.trees = {m: gpu.Octree(c.mesh, c.vs, max_items=m) for m in LEAF_SIZES}
    c.o = c.trees[16]
    c.aabbs, c.items = c.o.aabbs(), c.o.items()
    for o in c.trees.values():
        assert o.aabbs().tobytes() == c.aabbs.tobytes()      # the list does not depend on the leaf size
    gi = oracle.grid_info(c.v, c.vs)
    root_min = c.o.root_bounds()[0]
    assert np.array_equal(root_min, gi["bmin"])
    occ = np.unique(om.decode(c.items), axis=0)
    c.rays = np.ascontiguousarray(np.concatenate([family_rays(gi["dim"], root_min, c.vs, occ, seed=5),
                                                  zero_component_rays(gi, float(c.vs), 300, 7)]), F)
    c.rays.setflags(write=False)
    c.times = om.hit_times(c.aabbs, c.items, c.rays)
    c.times.setflags(write=False)
    return c


# ---- the lists and the counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,max_items", [(k, m) for m in LEAF_SIZES for k in KS] + [(k, 16) for k in MORE_KS])
@pytest.mark.parametrize("name,vs", ALL_SCENES)
def test_lists_and_counts(gpu, name, vs, k, max_items):
    c = _case(name, vs)
    o = c.trees[max_items]
    ref = mr.select(c.times, k)
    got = o.trace_multi(c.rays, max_hits=k)
    same(got, ref, "K=%d" % k)
    # the padding is exact (the reference pads; say so on the GPU's own arrays)
    pad = np.arange(k)[None, :] >= np.minimum(ref[2], k)[:, None]
    assert (got["t"][pad] == F(-1)).all() and (got["prim"][pad] == 0xFFFFFFFF).all()
    assert (got["t"][~pad] > 0).all()
    # slot 0 is the first-hit query's answer
    one = o.trace_ex(c.rays, want=("t", "prim"))
    assert np.array_equal(got["t"][:, 0].view(np.uint32), one["t"].view(np.uint32)) and np.array_equal(got["prim"][:, 0], one["prim"])
    # without the count the ray may stop early: the same lists
    same(o.trace_multi(c.rays, max_hits=k, want=("t", "prim")), ref, "K=%d, no count" % k)
    same(o.trace_multi(c.rays, max_hits=k, want=("count",)), ref, "K=%d, count only" % k)


def test_inputs_cover_duplicates_ties_and_overflow(gpu):
    for name, vs in ALL_SCENES:
        c = _case(name, vs)
        assert om.first_of_runs(c.items).sum() < len(c.items)
        cnt = mr.select(c.times, 1)[2]
        assert (cnt == 0).any() and (cnt > 3).any()
    t, p, _ = mr.select(_case(*om.TIE).times, 32)
    tie = (t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0)
    assert (tie.sum(axis=1) >= 4).sum() >= 8 and (p[:, 1:] > p[:, :-1])[tie].all()
    assert (mr.select(_case("cube", 0.0625).times, 1)[2] > 32).any()


def test_matches_the_bool_grid(gpu):
    """The distinct boxes of the octree are the Bool grid's: the same counts and the same t lists (prim differs: Morton order here)"""
    c = _case("rotcube", 0.09)
    g = gpu.Grid.voxelize(c.mesh, c.vs)
    for k in (3, 32):
        a, b = c.o.trace_multi(c.rays, max_hits=k), g.trace_multi(c.rays, max_hits=k)
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32))
    assert (a["count"] > 3).any()


@pytest.mark.parametrize("name,vs", [om.TIE, ("cube", 0.0625), ("adversarial", 0.1)])
def test_windows(gpu, name, vs):
    """tmin / tmax that cut the lists in the middle, bounds that ARE hit times (inclusive), and a tmax per ray"""
    c = _case(name, vs)
    pos = np.sort(c.times[c.times > 0])
    a, b = float(pos[int(0.35 * len(pos))]), float(pos[int(0.65 * len(pos))])
    for o in (c.trees[1], c.trees[100]):
        for k in (3, 32):
            ref = mr.select(c.times, k, tmin=a, tmax=b)
            same(o.trace_multi(c.rays, max_hits=k, tmin=a, tmax=b), ref, "window K=%d" % k)
            same(o.trace_multi(c.rays, max_hits=k, tmin=a, tmax=b, want=("t", "prim")), ref, "window K=%d, no count" % k)
        full_t = mr.select(c.times, 4)[0]
        tpr = np.where(full_t[:, 2] > 0, full_t[:, 2], F(10000.0)).astype(F)     # the third hit's own t: the list ends with it and its ties
        ref = mr.select(c.times, 8, tmax_per_ray=tpr)
        assert (ref[2] >= 3).any()
        same(o.trace_multi(c.rays, max_hits=8, tmax_per_ray=tpr), ref, "tmax_per_ray")
        same(o.trace_multi(c.rays, max_hits=8, tmax_per_ray=tpr, want=("t", "prim")), ref, "tmax_per_ray, no count")


def _paged_reference(times, k):
    """the whole lists, by paging the reference with K = k through the cursor"""
    n = len(times)
    at, ap = np.full(n, F(-1), F), np.zeros(n, np.uint32)
    ts, ps = [], []
    total = mr.select(times, 1)[2]
    for _ in range(int(-(-int(total.max()) // k)) + 1):
        t, p, _c = mr.select(times, k, after=(at, ap))
        ts.append(t)
        ps.append(p)
        last = np.maximum((t > 0).sum(axis=1) - 1, 0)
        have = t[:, 0] > 0
        at = np.where(have, t[np.arange(n), last], at).astype(F)
        ap = np.where(have, p[np.arange(n), last], ap).astype(np.uint32)
    return np.concatenate(ts, axis=1), np.concatenate(ps, axis=1), total


@pytest.mark.parametrize("name,vs", [om.TIE, ("cube", 0.0625)])
def test_paging_with_the_cursor(gpu, name, vs):
    """K = 3 (and K = 16) pages chained through `after` reassemble the whole lists and count down the totals"""
    c = _case(name, vs)
    ft, fp, cnt = _paged_reference(c.times, 32)
    n = len(c.rays)
    for k in (3, 16):
        at, ap = np.full(n, F(-1), F), np.full(n, 12345, np.uint32)   # (-1, anything) = no cursor
        pages_t, pages_p = [], []
        npages = -(-int(cnt.max()) // k) + 1
        for page in range(npages):
            got = c.o.trace_multi(c.rays, max_hits=k, after=(at, ap))
            same(got, mr.select(c.times, k, after=(at, ap)), "K=%d page %d" % (k, page))
            assert np.array_equal(got["count"], np.maximum(cnt.astype(np.int64) - k * page, 0))
            pages_t.append(got["t"])
            pages_p.append(got["prim"])
            last = np.maximum((got["t"] > 0).sum(axis=1) - 1, 0)
            have = got["t"][:, 0] > 0
            at = np.where(have, got["t"][np.arange(n), last], at).astype(F)
            ap = np.where(have, got["prim"][np.arange(n), last], ap).astype(np.uint32)
        gt, gp = np.concatenate(pages_t, axis=1), np.concatenate(pages_p, axis=1)
        w = int(cnt.max())
        assert gt.shape[1] >= w and ft.shape[1] >= w
        assert np.array_equal(gt[:, :w].view(np.uint32), ft[:, :w].view(np.uint32)) and np.array_equal(gp[:, :w], fp[:, :w])
        assert (gt[:, w:] == F(-1)).all() and (gp[:, w:] == 0xFFFFFFFF).all()
    # the early-out path under a cursor, in the middle of the lists
    mid_t, mid_p = np.where(cnt > 4, ft[:, 3], F(-1)).astype(F), np.where(cnt > 4, fp[:, 3], 0).astype(np.uint32)
    ref = mr.select(c.times, 3, after=(mid_t, mid_p))
    for o in c.trees.values():
        same(o.trace_multi(c.rays, max_hits=3, after=(mid_t, mid_p), want=("t", "prim")), ref, "cursor, no count")


# ---- where the dense grid cannot exist ---------------------------------------------------------------------------------------------------
def test_beyond_the_dense_cap(gpu):
    v, t = two_cluster_mesh()
    vs = F(1.0)
    mesh = gpu.Mesh.from_arrays(v, t)
    with pytest.raises(gpu.VxError) as e:
        gpu.Grid.voxelize(mesh, vs)
    assert e.value.status == CAPACITY
    rng = np.random.default_rng(4)
    n = 1500
    src = v.min(0) + rng.uniform(0, 1, (n, 3)) * (v.max(0) - v.min(0))
    tgt = np.where(rng.random((n, 1)) < 0.5, np.array([8.0, 8.0, 8.0]), np.array([6000.0, 6000.0, 6000.0])) + rng.uniform(-6, 6, (n, 3))
    d = tgt - src
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.concatenate([src, d], axis=1).astype(F), vx_scenes.random_rays(500, v.min(0), v.max(0), seed=6)])
    times = None
    for m in (16, 100):
        o = gpu.Octree(mesh, vs, max_items=m)
        if times is None:
            oa, items = o.aabbs(), o.items()
            assert 100 < len(oa) < 100_000
            times = om.hit_times(oa, items, rays)
            assert (mr.select(times, 1)[2][:n] > 3).mean() > 0.2
        for k in (8, 32):
            ref = mr.select(times, k)
            same(o.trace_multi(rays, max_hits=k), ref, "two clusters max_items=%d K=%d" % (m, k))
            same(o.trace_multi(rays, max_hits=k, want=("t", "prim")), ref, "two clusters max_items=%d K=%d, no count" % (m, k))


def test_axis_above_65535(gpu):
    """100 000 x 8 x 8 cells: cells that alias to one code (the low-16-bit interleave) form one run and count once"""
    v, t = long_thin_mesh()
    vs = F(1.0)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), vs)
    oa, items = o.aabbs(), o.items()
    assert oa["mx"][:, 0].max() <= 65536.0 + 1.0                 # aliased: no box beyond x = 65536
    rng = np.random.default_rng(3)
    n = 64                                                       # (rays x items stays below 10^8 in the brute force)
    x0 = np.concatenate([rng.uniform(0.0, 34_464.0, 32), rng.uniform(65_400.0, 65_700.0, 20), rng.uniform(66_000.0, 100_000.0, 12)])
    src = np.stack([x0, rng.choice([-6.0, 14.0], n), rng.uniform(0.0, 8.0, n)], 1)
    tgt = np.stack([x0 + rng.uniform(-30.0, 30.0, n), rng.uniform(0.0, 8.0, n), rng.uniform(0.0, 8.0, n)], 1)
    d = tgt - src
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([src, d], 1).astype(F)
    rays[56:] = [[65_300.0, 3.3, 4.1, 1.0, 0.001, 0.002]] * 8     # along x across the boundary at 65536, eight heights
    rays[56:, 1] += np.arange(8, dtype=F) * F(0.5)
    ref, with_duplicates = om.multi_blocked(oa, items, rays, 32)
    assert (ref[2] > 0).sum() >= 32 and (ref[2] > 32).any()
    assert (with_duplicates > ref[2]).any()                      # the runs matter on these rays
    same(o.trace_multi(rays, max_hits=32), ref, "long thin")
    same(o.trace_multi(rays, max_hits=32, want=("t", "prim")), ref, "long thin, no count")
    one = o.trace_ex(rays, want=("t", "prim"))
    assert np.array_equal(ref[0][:, 0].view(np.uint32), one["t"].view(np.uint32)) and np.array_equal(ref[1][:, 0], one["prim"])


# ---- camera rays, the device variant -------------------------------------------------------------------------------------------------------
def test_camera_rays(gpu):
    """Rays generated in the kernel against the same rays from the host (the rule of test_gpu_multihit.py: the same hit pattern, t within
    1e-5), and against the Bool grid's own camera query"""
    import oracle
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    mesh = gpu.Mesh.from_arrays(v, t)
    o = gpu.Octree(mesh, F(0.05))
    vi, pi = vx_scenes.camera_matrices(aspect=160.0 / 90.0)
    W, H = 160, 90
    cam = o.trace_multi(camera=(vi, pi, W, H), max_hits=8)
    exp = o.trace_multi(oracle.primary_rays(vi, pi, W, H), max_hits=8)
    assert (exp["count"] > 1).mean() > 0.01
    assert np.array_equal(cam["t"] > 0, exp["t"] > 0)
    assert np.allclose(cam["t"], exp["t"], rtol=0, atol=1e-5)
    grid = gpu.Grid.voxelize(mesh, F(0.05)).trace_multi(camera=(vi, pi, W, H), max_hits=8)
    assert np.array_equal(cam["t"].view(np.uint32), grid["t"].view(np.uint32)) and np.array_equal(cam["count"], grid["count"])


def test_device_variant_allocates_once(gpu):
    import torch
    c = _case("rotcube", 0.09)
    n, k = len(c.rays), 8
    d_rays = torch.from_numpy(np.array(c.rays)).cuda()
    d_t = torch.zeros((n, k), dtype=torch.float32, device="cuda")
    d_p = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run():
        c.o.trace_multi_device(d_rays.data_ptr(), n, k, d_t.data_ptr(), d_p.data_ptr(), d_c.data_ptr())
    run()
    before = gpu.device_allocations()
    run()
    run()
    assert gpu.device_allocations() == before
    torch.cuda.synchronize()
    host = c.o.trace_multi(c.rays, max_hits=k)
    dev = {"t": d_t.cpu().numpy(), "prim": d_p.cpu().numpy().view(np.uint32), "count": d_c.cpu().numpy().view(np.uint32)}
    same(dev, mr.select(c.times, k), "device")
    assert all(np.array_equal(dev[f].view(np.uint32), host[f].view(np.uint32)) for f in dev)
    # camera rays on the device variant: what the host variant gives
    vi, pi = vx_scenes.camera_matrices(eye=(4.0, 3.0, -2.0), ctr=(0.1, -0.07, 0.05), aspect=1.0)
    W = H = 24
    d_t2 = torch.zeros((W * H, k), dtype=torch.float32, device="cuda")
    d_c2 = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    c.o.trace_multi_device(None, 0, k, d_t2.data_ptr(), None, d_c2.data_ptr(), camera=(vi, pi, W, H))
    torch.cuda.synchronize()
    host = c.o.trace_multi(camera=(vi, pi, W, H), max_hits=k)
    assert (host["count"] > 0).any()
    assert np.array_equal(d_t2.cpu().numpy().view(np.uint32), host["t"].view(np.uint32))
    assert np.array_equal(d_c2.cpu().numpy().view(np.uint32), host["count"])


# ---- non-finite rays, NaN intervals ----------------------------------------------------------------------------------------------------------
def test_nonfinite_rays_and_nan_intervals(gpu):
    """Poisoned copies of hitting rays (tests/ray_nonfinite.py's poison_one) mixed into a batch of finite ones: count 0 and padded slots for
    them, the reference for their neighbours"""
    c = _case("rotcube", 0.09)
    k = 8
    ref = mr.select(c.times, k)
    hitting = np.flatnonzero(ref[2] > 0)
    base = hitting[np.linspace(0, len(hitting) - 1, 16).astype(int)]
    bad = np.ascontiguousarray(np.stack([r for j, b in enumerate(base) for _, r in rn.poison_one(np.array(c.rays[b]), j)]), F)
    assert rn.nonfinite(bad).all() and len(bad) > 500
    rng = np.random.default_rng(12)
    n = 1500
    dead = rng.random(n) < 0.35
    dead[[0, 63, 64, 127, n - 1]] = True          # first and last lanes of a wave, the batch's last ray
    dead[256:320] = True                          # one whole wave
    src = np.where(dead, -1, rng.integers(0, len(c.rays), n))
    rays = np.array(c.rays[np.maximum(src, 0)])
    rays[dead] = bad[rng.integers(0, len(bad), int(dead.sum()))]
    assert np.array_equal(rn.nonfinite(rays), dead)
    exp = rn.masked(src, {"t": ref[0], "prim": ref[1], "count": ref[2]})
    for o in (c.trees[1], c.trees[100]):
        for want in (("t", "prim", "count"), ("t", "prim"), ("count",)):
            got = o.trace_multi(rays, max_hits=k, want=want)
            for f in want:
                assert np.array_equal(got[f].view(np.uint32), exp[f].view(np.uint32)), (f, want)
        got = o.trace_multi(bad, max_hits=k)
        miss = rn.all_miss(len(bad), ("t", "prim", "count"), k)
        assert all(np.array_equal(got[f].view(np.uint32), miss[f].view(np.uint32)) for f in miss)
    # NaN in the interval accepts nothing
    o = c.o
    miss = rn.all_miss(len(c.rays), ("t", "prim", "count"), k)
    for kw in ({"tmin": np.nan}, {"tmax": np.nan}):
        for want in (("t", "prim", "count"), ("t", "prim")):
            got = o.trace_multi(c.rays, max_hits=k, want=want, **kw)
            assert all(np.array_equal(got[f].view(np.uint32), miss[f].view(np.uint32)) for f in want), kw
    tpr = np.full(len(c.rays), F(10000.0), F)
    tpr[::3] = F(np.nan)
    got = o.trace_multi(c.rays, max_hits=k, tmax_per_ray=tpr)
    live = ~np.isnan(tpr)
    for f, r in zip(("t", "prim", "count"), ref):
        assert np.array_equal(got[f][live].view(np.uint32), r[live].view(np.uint32))
        assert np.array_equal(got[f][~live].view(np.uint32), miss[f][~live].view(np.uint32))
    assert (ref[2][~live] > 0).any()


# ---- edges, errors, side effects -------------------------------------------------------------------------------------------------------------
def test_empty_octree_and_zero_rays(gpu):
    empty = gpu.Mesh.from_arrays(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    o = gpu.Octree(empty, F(0.1))
    rays = vx_scenes.random_rays(300, F([-1, -1, -1]), F([1, 1, 1]), seed=1)
    for want in (("t", "prim", "count"), ("t", "prim")):
        got = o.trace_multi(rays, max_hits=3, want=want)
        assert (got["t"] == F(-1)).all() and (got["prim"] == 0xFFFFFFFF).all() and not got.get("count", np.zeros(1)).any()
    o = _case("cube", 0.25).o
    got = o.trace_multi(np.zeros((0, 6), F), max_hits=4)
    assert got["t"].shape == (0, 4) and got["count"].shape == (0,)
    L = gpu.lib()
    a = gpu.MultiHitArgs()
    a.max_hits = 4
    assert L.vx_octree_trace_multi(o.h, C.byref(a)) == 0 and L.vx_octree_trace_multi_device(o.h, C.byref(a)) == 0
    one = np.zeros((1, 6), F)
    a.base.rays = one.ctypes.data
    assert L.vx_octree_trace_multi(o.h, C.byref(a)) == 0


def test_argument_errors_write_nothing(gpu):
    c = _case("cube", 0.25)
    L = gpu.lib()
    n = len(c.rays)
    t = np.full((n, 4), F(7), F)
    p = np.full((n, 4), 7, np.uint32)
    cnt = np.full(n, 7, np.uint32)
    junk = np.zeros(max(n, 16) * 3, F)

    def args():
        a = gpu.MultiHitArgs()
        a.base.rays, a.base.num_rays, a.base.tmin, a.base.tmax = c.rays.ctypes.data, n, 0.001, 10000.0
        a.base.t, a.base.prim, a.count, a.max_hits = t.ctypes.data, p.ctypes.data, cnt.ctypes.data, 4
        return a

    for fn in (L.vx_octree_trace_multi, L.vx_octree_trace_multi_device):
        assert fn(None, C.byref(args())) == INVALID_ARG
        assert fn(c.o.h, None) == INVALID_ARG
        for k in (0, 33, 0xFFFFFFFF):
            a = args()
            a.max_hits = k
            assert fn(c.o.h, C.byref(a)) == INVALID_ARG, k
        a = args()
        a.after_t = junk.ctypes.data
        assert fn(c.o.h, C.byref(a)) == INVALID_ARG
        a = args()
        a.after_prim = junk.ctypes.data
        assert fn(c.o.h, C.byref(a)) == INVALID_ARG
        for field in ("normal", "shadowed", "hits", "num_hits"):
            a = args()
            setattr(a.base, field, junk.ctypes.data)
            assert fn(c.o.h, C.byref(a)) == INVALID_ARG, field
        a = args()
        a.base.any_hit = 1
        assert fn(c.o.h, C.byref(a)) == INVALID_ARG
        a = args()
        a.base.rays = None     # rays announced, but neither a buffer nor a camera
        assert fn(c.o.h, C.byref(a)) == INVALID_ARG
    assert (t == F(7)).all() and (p == 7).all() and (cnt == 7).all()


def test_each_query_queues_its_own_kernel(gpu):
    c = _case("rotcube", 0.09)
    gpu.profile_enable(True)
    gpu.profile_reset()
    c.o.trace(c.rays)
    names = list(gpu.profile_read())
    assert "k_octree_trace" in names and not any(n.startswith("k_octree_multihit") for n in names), names
    gpu.profile_reset()
    c.o.trace_multi(c.rays, max_hits=8)
    c.o.trace_multi(c.rays, max_hits=32)
    prof = gpu.profile_read()   # (kernel names come without their template arguments)
    gpu.profile_enable(False)
    assert prof["k_octree_multihit"][1] == 2 and "k_octree_trace" not in prof, prof


# ---- C++ facade and CLI -----------------------------------------------------------------------------------------------------------------
def run(cmd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = PKG + ":" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)


def test_facade_trace_multi(gpu, tmp_path):
    import build as vxbuild
    exe = str(tmp_path / "octree_multihit_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "octree_multihit_facade.cpp"), "-o", exe, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    v, t = vx_scenes.rotated_cube()
    obj = tmp_path / "c.obj"
    vx_scenes.write_obj(str(obj), v, t)
    vs = F(0.09)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), vs)
    rays = vx_scenes.random_rays(200, v.min(0), v.max(0), seed=8)
    rays.tofile(str(tmp_path / "rays.bin"))
    k, tmin, tmax = 5, 0.001, 10000.0
    r = run([exe, str(obj), repr(float(vs)), str(tmp_path / "rays.bin"), str(tmp_path / "out.bin"), str(k), repr(tmin), repr(tmax)])
    assert r.returncode == 0, r.stdout
    ref = om.multi(o.aabbs(), o.items(), rays, k, tmin=tmin, tmax=tmax)
    assert (ref[2] > k).any() and (ref[2] == 0).any()
    raw = np.fromfile(str(tmp_path / "out.bin"), np.uint32)
    n = len(rays)
    assert len(raw) == 2 * n * k + n
    got = {"t": raw[: n * k].view(F).reshape(n, k), "prim": raw[n * k: 2 * n * k].reshape(n, k), "count": raw[2 * n * k:]}
    same(got, ref, "facade")


def test_cli_octree_xray(gpu, tmp_path):
    """--grid octree --octree-xray: a 16-bit PGM of min(count, 65535) per camera ray, against Octree.trace_multi with the camera the CLI used"""
    v, t = vx_scenes.cube()
    obj = tmp_path / "cube.obj"
    vx_scenes.write_obj(str(obj), v, t)
    pgm, cam = tmp_path / "x.pgm", tmp_path / "cam.bin"
    W, H = 96, 54
    exe = os.path.join(PKG, "voxilizer")
    r = run([exe, str(obj), "0.0625", "--grid", "octree", "--octree-xray", str(pgm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)])
    assert r.returncode == 0 and "xray %dx%d" % (W, H) in r.stdout, r.stdout
    raw = open(pgm, "rb").read()
    hdr = b"P5\n%d %d\n65535\n" % (W, H)
    assert raw.startswith(hdr) and len(raw) == len(hdr) + 2 * W * H
    img = np.frombuffer(raw[len(hdr):], ">u2").reshape(H, W)
    cm = np.fromfile(cam, F)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), F(0.0625))
    cnt = o.trace_multi(camera=(cm[:16], cm[16:], W, H), max_hits=1, want=("count",))["count"].reshape(H, W)
    assert np.array_equal(img, np.minimum(cnt, 65535))
    assert cnt.max() >= 4 and (cnt == 0).any()
    r = run([exe, str(obj), "0.0625", "--octree-xray", str(pgm)])
    assert r.returncode == 2 and "--octree-xray" in r.stdout
    for extra in (["--gpus", "2"], ["--bench", "1"]):
        r = run([exe, str(obj), "0.0625", "--grid", "octree", "--octree-xray", str(pgm)] + extra)
        assert r.returncode == 2 and "--octree-xray" in r.stdout, r.stdout
