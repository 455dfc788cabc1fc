"""GPU tests of the triangle tracers where their LDS stack is full and where all of a tie falls to the index part of the key: the chain
scenes, stacked triangles and coincident instances of tests/deep_trees.py.  k_bvh_trace, k_bvh_multihit, k_tlas_trace and k_tlas_multihit
size the stack [level][lane] to the height the build reports (the TLAS: its height bound plus the tallest BLAS) and nothing checks the
index at run time: a height reported one too low, or a bound off by one, loses a subtree only on a ray that holds `height` entries at
once.  The rays here do (deep_trees.stack_model shows it on the very node arrays the library returns); every result is compared bit for
bit with the brute force over all triangles (tests/mesh_ref.py, mesh_multihit_ref.py, instance_ref.py)."""
import functools

import numpy as np
import pytest

import deep_trees as dt
import instance_ref
import mesh_multihit_ref as mm
import mesh_ref
import vx_scenes
from test_gpu_mesh_multihit import ALL, ALL_TLAS, same
from test_gpu_mesh_trace import check_closest, check_structure, vertex_rays

pytestmark = pytest.mark.gpu

F = np.float32
LEAF_SIZES = (1, 4, 0)          # 0 = the library default
KS = (1, 8, 32)
SCENES = [(m, mirrored) for mirrored in (False, True) for m in dt.CLUSTERS]     # mirrored: a ray holds every level (deep_trees.chain_scene)


@functools.lru_cache(maxsize=None)
def chain_bvh(m, mirrored, max_leaf):
    import voxhip as gpu
    sc = dt.chain_scene(m, mirrored)
    return gpu.Mesh.from_arrays(sc.v, sc.t).bvh(max_leaf=max_leaf)


@functools.lru_cache(maxsize=None)
def chain_tlas(tall):
    import voxhip as gpu
    ci = dt.chain_instances(tall)
    bl = [gpu.Mesh.from_arrays(v, t).bvh() for v, t in ci.meshes]
    return gpu.Tlas(bl, ci.inst)


def bits(a):
    return a.view(np.uint32) if a.dtype == F else a


# ---- one BVH ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", LEAF_SIZES)
@pytest.mark.parametrize("m,mirrored", SCENES)
def test_bvh_height_is_the_radix_height(gpu, m, mirrored, max_leaf):
    sc = dt.chain_scene(m, mirrored)
    b = chain_bvh(m, mirrored, max_leaf)
    h = dt.radix_height(dt.bvh_keys(sc.v, sc.t))
    assert b.height == h and b.num_ill_conditioned == 0
    depth = check_structure(b, sc.v, sc.t)
    if max_leaf == 1:       # every node survives the collapse: the node array is the radix tree
        assert depth == h and b.num_nodes == 2 * len(sc.t) - 1
        rays = dt.deep_rays(m, mirrored)[dt.DIAGONAL][:6]
        held = [dt.most_held(b.nodes(), rays, left_on_tie=left) for left in (True, False)]
        print("%s: %d triangles, height %d, most stack entries held %s" % (sc.name, len(sc.t), h, held))
        assert min(held) >= h - (1 if mirrored else dt.STACK_MARGIN)
        if mirrored and m == 1:     # one entry per interior node of the longest path: a stack one level short loses a subtree here
            assert min(held) == h


@pytest.mark.parametrize("max_leaf", LEAF_SIZES)
@pytest.mark.parametrize("m,mirrored", SCENES)
def test_bvh_first_hit_on_the_chain(gpu, m, mirrored, max_leaf):
    sc = dt.chain_scene(m, mirrored)
    b = chain_bvh(m, mirrored, max_leaf)
    rays = dt.deep_rays(m, mirrored)
    ref = dt.chain_closest(m, mirrored)
    assert (ref[0][dt.DIAGONAL] > 0).all() and 0 < (ref[0] > 0).sum() < len(rays)
    check_closest(b, sc.v, sc.t, rays, "%s max_leaf=%d" % (sc.name, max_leaf), ref)
    sh = b.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"]
    assert np.array_equal(sh, mesh_ref.any_hit(sc.v, sc.t, rays))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("max_leaf", LEAF_SIZES)
@pytest.mark.parametrize("m,mirrored", SCENES)
def test_bvh_lists_and_counts_on_the_chain(gpu, m, mirrored, max_leaf, k):
    """the count query prunes nothing: it is the one that holds the whole stack"""
    sc = dt.chain_scene(m, mirrored)
    b = chain_bvh(m, mirrored, max_leaf)
    rays = dt.deep_rays(m, mirrored)
    what = "%s max_leaf=%d K=%d" % (sc.name, max_leaf, k)
    ref = mm.select(dt.chain_hits(m, mirrored), k)
    same(b.trace_multi(rays, max_hits=k, want=("count",)), ref, what + ", count only")
    same(b.trace_multi(rays, max_hits=k, want=("t", "prim", "bary")), ref, what + ", lists only")
    same(b.trace_multi(rays, max_hits=k, want=ALL), ref, what)
    tm = dt.chain_tmax(m, mirrored)        # the middle hit's own t: the list ends in the middle of the chain, with that hit
    cut = mm.select(mm.all_hits(sc.v, sc.t, rays, tmax_per_ray=tm), k)
    assert (cut["count"][dt.DIAGONAL] < ref["count"][dt.DIAGONAL]).all() and (cut["count"][dt.DIAGONAL] > 0).all()
    same(b.trace_multi(rays, max_hits=k, tmax_per_ray=tm, want=ALL), cut, what + ", tmax per ray")


def test_bvh_rebuild_follows_the_height(gpu):
    """one handle: the tall chain, a cube (short), the chain again -- the stack is sized by the height of the build that is traced"""
    sc = dt.chain_scene(4096)
    cv, ct = vx_scenes.scene("rotcube")
    big, small = gpu.Mesh.from_arrays(sc.v, sc.t), gpu.Mesh.from_arrays(cv, ct)
    crays = np.concatenate([vx_scenes.random_rays(200, cv.min(0), cv.max(0), seed=3), vertex_rays(cv, ct, 100, 4)])
    b = big.bvh(max_leaf=1)
    tall = b.height
    assert tall == dt.radix_height(dt.bvh_keys(sc.v, sc.t))
    for _ in range(2):
        b.build_into(small)
        assert b.height == dt.radix_height(dt.bvh_keys(cv, ct)) == small.bvh(max_leaf=1).height < tall and b.num_triangles == len(ct)
        check_closest(b, cv, ct, crays, "rebuilt as rotcube")
        b.build_into(big)
        assert b.height == tall and check_structure(b, sc.v, sc.t) == tall
        check_closest(b, sc.v, sc.t, dt.deep_rays(4096), "rebuilt as the chain", dt.chain_closest(4096))
        same(b.trace_multi(dt.deep_rays(4096), max_hits=8, want=ALL), mm.select(dt.chain_hits(4096), 8), "rebuilt as the chain")


# ---- a run of equal t longer than K ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", LEAF_SIZES)
def test_stacked_first_hit_and_pages(gpu, max_leaf):
    sc = dt.stacked_scene(100)
    hits = dt.stacked_hits(100)
    b = gpu.Mesh.from_arrays(sc.v, sc.t).bvh(max_leaf=max_leaf)
    assert b.height == dt.radix_height(dt.bvh_keys(sc.v, sc.t))
    rt, rp = check_closest(b, sc.v, sc.t, sc.rays, "stacked max_leaf=%d" % max_leaf)
    hit = rt > 0
    assert hit.sum() >= 90 and (rp[hit] == 0).all()                  # the lowest index of the run of 100
    k, n = 32, len(sc.rays)
    total = mm.select(hits, 1)["count"]
    assert set(np.unique(total)) == {0, 200}
    cur = (np.full(n, F(-1), F), np.zeros(n, np.uint32))
    pages = []
    for page in range(8):                                            # 7 pages of 32 hold the 200 hits; the 8th is empty
        got = b.trace_multi(sc.rays, max_hits=k, after=cur, want=ALL)
        same(got, mm.select(hits, k, after=cur), "page %d" % page)
        assert np.array_equal(got["count"], np.maximum(total.astype(np.int64) - k * page, 0))    # what remains strictly after the cursor
        pages.append(got)
        cur = mm.cursor_of(got, cur)
    assert not pages[-1]["count"].any() and (pages[-1]["t"] == F(-1)).all()
    whole = mm.select(hits, 8 * k)
    for f in ("t", "prim", "bary"):
        assert np.array_equal(bits(np.concatenate([p[f] for p in pages], axis=1)), bits(whole[f]))
    assert np.array_equal(whole["prim"][hit][:, :200], np.tile(np.arange(200, dtype=np.uint32), (hit.sum(), 1)))


@pytest.mark.parametrize("max_leaf", LEAF_SIZES)
def test_stacked_cursor_inside_a_run(gpu, max_leaf):
    """a cursor (t, prim = 49) in the middle of 100 equal t: all of `strictly after` falls to the prim part"""
    sc = dt.stacked_scene(100)
    hits = dt.stacked_hits(100)
    b = gpu.Mesh.from_arrays(sc.v, sc.t).bvh(max_leaf=max_leaf)
    first = mm.select(hits, 200)
    hit = first["count"] == 200
    n = len(sc.rays)
    for prim, slot, left in ((49, 49, 150), (99, 99, 100), (149, 149, 50), (199, 199, 0), (0, 0, 199)):
        cur = (np.where(hit, first["t"][:, slot], F(-1)).astype(F), np.full(n, prim, np.uint32))
        for k in (1, 32):
            got = b.trace_multi(sc.rays, max_hits=k, after=cur, want=ALL)
            same(got, mm.select(hits, k, after=cur), "cursor at prim %d, K=%d" % (prim, k))
            assert (got["count"][hit] == left).all()
            if left:
                assert (got["prim"][hit, 0] == prim + 1).all()
    # a prim beyond the run on the near layer's t: nothing of the near run is left, the far run is whole
    cur = (np.where(hit, first["t"][:, 0], F(-1)).astype(F), np.full(n, 0xFFFFFFFE, np.uint32))
    got = b.trace_multi(sc.rays, max_hits=8, after=cur, want=ALL)
    same(got, mm.select(hits, 8, after=cur), "cursor behind the run")
    assert (got["count"][hit] == 100).all() and (got["prim"][hit, 0] == 100).all()


# ---- the TLAS -------------------------------------------------------------------------------------------------------------------------------
def check_tlas(tl, meshes, inst, rays, what, hits=None):
    rt, ri, rp, rb = instance_ref.closest(meshes, inst, rays)
    got = tl.trace_ex(rays, want=("t", "instance", "prim", "bary"))
    same(got, {"t": rt, "instance": ri, "prim": rp, "bary": rb}, what)
    sh = tl.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"]
    assert np.array_equal(sh, instance_ref.any_hit(meshes, inst, rays)), what
    hits = mm.all_hits_tlas(meshes, inst, rays) if hits is None else hits
    same(tl.trace_multi(rays, max_hits=32, want=ALL_TLAS), mm.select(hits, 32), what + ", K=32")
    same(tl.trace_multi(rays, max_hits=32, want=("count",)), mm.select(hits, 32), what + ", count only")
    return rt, hits


@pytest.mark.parametrize("n", dt.PURE_CHAIN_N)
def test_tlas_pure_chain_reaches_the_bound(gpu, n):
    """n - 1 is the binding branch of the height bound for every n <= 35: here the tree really is that tall"""
    pc = dt.pure_chain_instances(n)
    tl = gpu.Tlas([gpu.Mesh.from_arrays(*pc.meshes[0]).bvh()], pc.inst)
    nodes = tl.nodes()
    assert tl.height() == dt.node_depth(nodes) == n - 1 == dt.tlas_height_bound(n) and dt.is_chain(nodes)
    assert dt.most_held(nodes, pc.rays[dt.DIAGONAL][:6]) == n - 1
    rt, _ = check_tlas(tl, pc.meshes, pc.inst, pc.rays, "pure chain of %d" % n)
    assert (rt[dt.DIAGONAL] > 0).all()


@pytest.mark.parametrize("tall", [False, True])
def test_tlas_chain(gpu, tall):
    """27 instances in a chain of height 26 = n - 1; tall: each a BLAS of height 38, so that the stack holds both at once"""
    ci = dt.chain_instances(tall)
    tl = chain_tlas(tall)
    nodes = tl.nodes()
    h = tl.height()
    assert h == dt.node_depth(nodes) == dt.radix_height(dt.tlas_keys(ci.meshes, ci.inst)) and h <= dt.tlas_height_bound(len(ci.inst))
    assert h == 26 and dt.is_chain(nodes)
    leaf = (nodes["b"] & np.uint32(dt.LEAF)) != 0
    assert np.array_equal(np.sort(nodes["a"][leaf]), np.arange(len(ci.inst)))
    held = [dt.most_held(nodes, ci.rays[dt.DIAGONAL][:6], left_on_tie=left) for left in (True, False)]
    bh = tl.blas[0].height
    print("chain_instances(tall=%s): TLAS height %d (bound %d), most TLAS stack entries held %s, BLAS height %d" % (tall, h, dt.tlas_height_bound(len(ci.inst)), held, bh))
    assert min(held) >= h - dt.STACK_MARGIN
    assert bh == (38 if tall else 0)
    rt, hits = check_tlas(tl, ci.meshes, ci.inst, ci.rays, "chain instances, tall=%s" % tall)
    assert (rt[dt.DIAGONAL] > 0).all()
    assert np.bincount(hits.ray, minlength=hits.n).max() > (32 if tall else 20)


def test_tlas_coincident_instances(gpu):
    """64 instances under one transform: every hit is a 64-fold tie that only the instance index orders"""
    co = dt.coincident_instances(64)
    tl = gpu.Tlas([gpu.Mesh.from_arrays(*co.meshes[0]).bvh()], co.inst)
    assert tl.height() == dt.node_depth(tl.nodes()) <= dt.tlas_height_bound(64)
    rt, hits = check_tlas(tl, co.meshes, co.inst, co.rays, "coincident")
    hit = rt > 0
    assert hit.sum() >= 30
    one = tl.trace_ex(co.rays, want=("instance", "prim"))
    assert (one["instance"][hit] == 0).all() and (one["prim"][hit] == 0).all()
    n, k = len(co.rays), 32
    total = mm.select(hits, 1)["count"]
    cur = (np.full(n, F(-1), F), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    pages = []
    for page in range(3):
        got = tl.trace_multi(co.rays, max_hits=k, after=cur, want=ALL_TLAS)
        same(got, mm.select(hits, k, after=cur), "page %d" % page)
        assert np.array_equal(got["count"], np.maximum(total.astype(np.int64) - k * page, 0))
        pages.append(got)
        cur = mm.cursor_of(got, cur, tlas=True)
    assert not pages[-1]["count"].any()
    inst = np.concatenate([p["instance"] for p in pages[:2]], axis=1)
    assert np.array_equal(inst[hit], np.tile(np.arange(64, dtype=np.uint32), (hit.sum(), 1)))
    for i in (0, 31, 40, 62, 63):          # a cursor inside the run resumes at the next instance
        cur = (np.where(hit, rt, F(-1)).astype(F), np.full(n, i, np.uint32), np.zeros(n, np.uint32))
        got = tl.trace_multi(co.rays, max_hits=k, after=cur, want=ALL_TLAS)
        same(got, mm.select(hits, k, after=cur), "cursor at instance %d" % i)
        assert (got["count"][hit] == 63 - i).all()
        if i < 63:
            assert (got["instance"][hit, 0] == i + 1).all()


def test_tlas_update_between_chain_and_scatter(gpu):
    """one handle: the chain (height 26), 64 scattered instances (short), the chain again -- equal to a fresh TLAS each time"""
    ci = dt.chain_instances(False)
    rnd = dt.random_instances(64)
    bl = [gpu.Mesh.from_arrays(*ci.meshes[0]).bvh()]
    rays = np.concatenate([ci.rays, vx_scenes.random_rays(300, F([0, 0, 0]), F([1, 1, 1]), seed=43)]).astype(F)
    tl = gpu.Tlas(bl, ci.inst)
    for inst in (rnd, ci.inst, rnd, ci.inst):
        tl.update(inst)
        fresh = gpu.Tlas(bl, inst)
        assert tl.height() == fresh.height() and np.array_equal(tl.nodes().view(np.uint32), fresh.nodes().view(np.uint32))
        want = ("t", "instance", "prim", "bary", "normal")
        same(tl.trace_ex(rays, want=want), fresh.trace_ex(rays, want=want), "updated")
        same(tl.trace_multi(rays, max_hits=32, want=ALL_TLAS), fresh.trace_multi(rays, max_hits=32, want=ALL_TLAS), "updated, K=32")
    assert tl.height() == 26
    rt, ri, rp, rb = instance_ref.closest(ci.meshes, ci.inst, rays)
    same(tl.trace_ex(rays, want=("t", "instance", "prim", "bary")), {"t": rt, "instance": ri, "prim": rp, "bary": rb}, "back on the chain")
    rt, ri, rp, rb = instance_ref.closest(ci.meshes, rnd, rays)
    assert (rt > 0).sum() >= 10
    tl.update(rnd)
    same(tl.trace_ex(rays, want=("t", "instance", "prim", "bary")), {"t": rt, "instance": ri, "prim": rp, "bary": rb}, "scattered")
