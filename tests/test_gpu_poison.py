"""Every feature on poisoned pool blocks (vx_pool_poison).  A block the library's pool hands out holds what its previous owner left; with
the mode on it holds a known pattern instead -- 0xFFFFFFFF (the sentinel, -1, a NaN, the newest scan generation), 0xA5A5A5A5, 0x00000001
(counters off by one, flags that look set) -- so a kernel that reads a word nobody wrote computes from the pattern and its output differs
from the reference.  Every handle is created after the mode is switched on; every output is compared with the reference the feature's own
test file uses (tests/*_ref.py, oracle.py), bit for bit or at that file's tolerance, never with another run of the library; and every test
asserts that the mode did fill each block the test requested.  Shapes: tests/stale_cases.py."""
import contextlib
import functools

import numpy as np
import pytest

import deep_trees as dt
import instance_ref
import mesh_multihit_cases as mc
import mesh_multihit_ref as mm
import mesh_ref
import multihit_ref as mr
import octree_multihit_ref as om
import oracle
import reference_cases as rc
import render_ref
import scan_ref as sr
import stale_cases as sc
import vx_scenes
from test_gpu_attributes import bvh_reference as attr_bvh_reference, check as attr_check, write_textured_plane
from test_gpu_instance_frames import check as inst_check, instanced_scene, reference as inst_reference
from test_gpu_instances import check as tlas_check
from test_gpu_mesh_multihit import ALL, ALL_TLAS, same as same_mesh_hits
from test_gpu_mesh_trace import check_closest, write_mesh_obj
from test_gpu_multihit import same as same_hits
from test_gpu_parity import _value_ids
from test_gpu_render import check_frame, reference as frame_reference
from test_gpu_scan import TAG, check as scan_check, expect_path
from test_gpu_solid import check_solid, expected as solid_expected, scene as solid_scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
patterns = pytest.mark.parametrize("pattern", sc.PATTERNS, ids=["%08X" % p for p in sc.PATTERNS])


@pytest.fixture(scope="module", autouse=True)
def poison_off(gpu):
    try:
        yield
    finally:
        gpu.pool_poison(None)


@contextlib.contextmanager
def poisoned(gpu, pattern):
    """the mode on with `pattern`; at the end: every block requested in between was filled, and there was one"""
    gpu.pool_poison(pattern)
    a0, p0 = gpu.device_allocations(), gpu.pool_poisoned_blocks()
    yield
    a1, p1 = gpu.device_allocations(), gpu.pool_poisoned_blocks()
    assert p1 - p0 == a1 - a0, "poisoned %d of %d requested blocks" % (p1 - p0, a1 - a0)
    assert p1 > p0, "the test requested no block: the mode was not exercised"


# ---- references: computed once, shared, left unchanged (tests/stale_cases.py) -----------------------------------------------------------------
Ref, soup_ref, soup_rays, mask_ref, check_build, kinds = sc.Ref, sc.soup_ref, sc.soup_rays, sc.mask_ref, sc.check_build, sc.kinds


def camera(eye, ctr):
    vi, pi = vx_scenes.camera_matrices(eye=eye, ctr=ctr, aspect=W / H)
    return vi, pi, W, H


# ---- 1. voxelize ---------------------------------------------------------------------------------------------------------------------------
@patterns
def test_voxelize(gpu, pattern):
    with poisoned(gpu, pattern):
        for dims in (sc.LARGE, sc.SMALL):
            v, t = sc.soup(dims)
            mesh = gpu.Mesh.from_arrays(v, t)
            for sat in (0, 1):
                r = soup_ref(dims, sat)
                for kind in kinds(gpu):
                    check_build(gpu, gpu.Grid.voxelize(mesh, sc.SOUP_VS, kind, sat_variant=sat), kind, r, "%s kind %d sat %d" % (dims, kind, sat))
        # cases of the reference-parity tests: lattice planes where the candidate range rounds either way, one triangle, no faces
        for name, vs in (("lattice01", 0.1), ("lattice007", 0.07), ("single", 0.05), ("nofaces", 0.09)):
            v, t = rc.scene(name)
            mesh = gpu.Mesh.from_arrays(v, t)
            for mode, kind in zip(rc.SERIAL_MODES, kinds(gpu)):
                e = rc.expected(v, t, F(vs), mode, 2)
                g = gpu.Grid.voxelize(mesh, F(vs), kind)
                what = "%s %s" % (name, mode)
                assert g.aabbs().tobytes() == e["aabbs"].tobytes() and g.memory_bytes() == e["memory_bytes"], what
                assert g.describe()["set_calls"] == e["calls"], what
                if e["occ"] is not None:
                    assert np.array_equal(g.bitmask(), e["occ"]), what
        r = soup_ref(sc.LARGE)
        mesh = gpu.Mesh.from_arrays(r.v, r.t)
        # per-voxel materials
        recs, ids = sc.material_records(gpu, len(r.t))
        mesh.set_materials(recs, ids)
        for kind in kinds(gpu):
            g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, kind, materials=True)
            check_build(gpu, g, kind, r, "materials kind %d" % kind)
            sc.check_material_ids(gpu, g, kind, r, recs, ids)
        # solid
        g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, gpu.GRID_BOOL, solid=True)
        check_solid(gpu, g, gpu.GRID_BOOL, r.v, r.t, sc.SOUP_VS, 0, solid_expected(r.v, r.t, sc.SOUP_VS, 0))
        # a list left to the next ray batch: the rebuild, the batch, then the list
        rays = soup_rays(sc.LARGE)
        ot, op = oracle.trace_brute(r.boxes, rays)                   # (prim is the occupied cell's rank, whatever the flavour)
        g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, gpu.GRID_VEC)
        for _ in range(2):
            g.revoxelize(mesh, sc.SOUP_VS, list_async=True)
            tt, pp, nh = g.trace(rays)
            assert np.array_equal(tt, ot) and np.array_equal(pp, op) and nh == int((ot > 0).sum()), "list_async: the ray batch"
            check_build(gpu, g, gpu.GRID_VEC, r, "list_async")
        # word shards and triangle ranges
        acc = np.zeros_like(r.words)
        for rank in range(3):
            b, e, _ = gpu.shard_words(len(r.words), rank, 3)
            w = gpu.Grid.voxelize(mesh, sc.SOUP_VS, words=(b, e)).bitmask()
            assert not w[:b].any() and not w[e:].any() and np.array_equal(w[b:e], r.words[b:e]), "word shard %d" % rank
            acc |= w
            w = gpu.Grid.voxelize(mesh, sc.SOUP_VS, shard=(rank, 3)).bitmask()
            assert not w[:b].any() and not w[e:].any() and np.array_equal(w[b:e], r.words[b:e]), "rank shard %d" % rank
        assert np.array_equal(acc, r.words)
        parts = []
        for rank in range(3):
            b, e = gpu.shard_range(len(r.t), rank, 3)
            parts.append(gpu.Grid.voxelize(mesh, sc.SOUP_VS, gpu.GRID_VEC, tris=(b, e)).aabbs())
        assert np.concatenate(parts).tobytes() == r.vec.tobytes(), "triangle ranges"
        # VoxelGrid ctor + setVoxel + getAabbs
        cells = sc.mask("small_tenth")
        pts = np.argwhere(cells)[:, ::-1]
        for kind in kinds(gpu):
            g = gpu.Grid.create(kind, *sc.SMALL, sc.VS, sc.ORG)
            for x, y, z in pts.tolist():
                g.set_voxel(x, y, z)
            sc.check_mask(g, cells, "setVoxel kind %d" % kind)
            sc.check_bool_list(g, cells, "setVoxel kind %d" % kind)   # (ascending cells: the Vec list's insertion order is the same)
            assert g.describe()["set_calls"] == len(pts)


# ---- 2. several ranks ----------------------------------------------------------------------------------------------------------------------
@patterns
def test_voxelize_multi(gpu, pattern):
    with poisoned(gpu, pattern):
        r = soup_ref(sc.LARGE)
        mesh = gpu.Mesh.from_arrays(r.v, r.t)
        recs, ids = sc.material_records(gpu, len(r.t))
        mesh.set_materials(recs, ids)
        tv, nvalues, _ = _value_ids(recs, ids)
        oids, order = oracle.material_ids(r.v, r.t, sc.SOUP_VS, tv, nvalues)
        rays = soup_rays(sc.LARGE)
        ot, op = oracle.trace_brute(r.boxes, rays)
        for all_gather in (False, True):
            grids = gpu.Grid.voxelize_multi(mesh, sc.SOUP_VS, [0, 0], all_gather=all_gather)   # device 0 twice: a rehearsal on one device
            assert len(grids) == (2 if all_gather else 1)
            for g in grids:
                check_build(gpu, g, gpu.GRID_BOOL, r, "voxelize_multi")
                tt, pp, _ = g.trace(rays)
                assert np.array_equal(tt, ot) and np.array_equal(pp, op)
        m = gpu.Multi(mesh, [0, 0])
        for mats, all_gather in ((False, False), (True, True), (True, False)):
            for g in m.voxelize(sc.SOUP_VS, materials=mats, all_gather=all_gather):
                check_build(gpu, g, gpu.GRID_BOOL, r, "Multi")
                gm, gid = g.materials()
                if mats:
                    assert np.array_equal(gid, oids) and len(gm) == len(order)
                else:
                    assert len(gid) == 0
        small = soup_ref(sc.SMALL)
        ms = gpu.Multi(gpu.Mesh.from_arrays(small.v, small.t), [0, 0, 0])   # after the large mesh: another context, fewer words than a tile
        for g in ms.voxelize(sc.SOUP_VS, all_gather=True):
            check_build(gpu, g, gpu.GRID_BOOL, small, "Multi, small")
        ms.free()
        m.free()


# ---- 3. octree build -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def octree_ref(dims, max_items):
    r = soup_ref(dims)
    return oracle.octree(r.v, r.t, sc.SOUP_VS, max_items=max_items, threads=2)


def check_octree(o, ref, what=""):
    assert o.num_items == len(ref["items"]) and o.num_nodes == len(ref["nodes"]), what
    assert np.array_equal(o.items(), ref["items"]), what + ": items"
    assert o.nodes().tobytes() == ref["nodes"].tobytes(), what + ": nodes"
    assert o.aabbs().tobytes() == ref["aabbs"].tobytes(), what + ": aabbs"
    assert o.memory_bytes() == ref["bytes"]
    mn, mx = o.root_bounds()
    assert np.array_equal(mn, ref["root_min"]) and np.array_equal(mx, ref["root_max"]), what + ": root bounds"


GROWN_VS, GROWN_ITEMS = F(1.0 / 64), 65   # 37 037 items, 2 970 nodes (846 at the next smaller candidate, soup(4000))


def grown_soup():
    return vx_scenes.soup(5000, seed=4, edge=1.5 / 64)


@functools.lru_cache(maxsize=None)
def grown_ref():
    """the oracle's sorted items of grown_soup() and Octree::buildTree on them (test_gpu_parity.test_octree_node_array_large's reference)"""
    v, t = grown_soup()
    h = oracle.hits(v, t, GROWN_VS, threads=2, sat=0)
    items = np.sort(oracle.morton3d_np(h[:, 0], h[:, 1], h[:, 2]))
    bits = int(np.ceil(np.log2(max(oracle.grid_info(v, GROWN_VS)["dim"]))))
    return items, oracle.octree_nodes_from_sorted_items(items, bits, GROWN_ITEMS)


@patterns
def test_octree_build(gpu, pattern):
    with poisoned(gpu, pattern):
        for dims in (sc.LARGE, sc.SMALL):
            r = soup_ref(dims)
            mesh = gpu.Mesh.from_arrays(r.v, r.t)
            for max_items in (16, 1, 100):   # the direct node-array form (<= 64) and the level-by-level form
                check_octree(gpu.Octree(mesh, sc.SOUP_VS, max_items), octree_ref(dims, max_items), "%s max_items %d" % (dims, max_items))
        # the level-by-level form past its first blocks of 1024 nodes: the arrays indexed by breadth-first id grow and keep their contents
        o = gpu.Octree(gpu.Mesh.from_arrays(*grown_soup()), GROWN_VS, GROWN_ITEMS)
        items, nodes = grown_ref()
        assert len(nodes) > 2048
        assert np.array_equal(o.items(), items)
        assert o.num_nodes == len(nodes) and o.nodes().tobytes() == nodes.tobytes()


# ---- 4. first hits on the grid -------------------------------------------------------------------------------------------------------------
@patterns
def test_trace_ex(gpu, pattern):
    import torch
    with poisoned(gpu, pattern):
        for name in ("large_half", "small_tenth"):
            r = mask_ref(name)
            g = sc.masked_grid(gpu, r.cells)
            ot, op = oracle.trace_brute(r.boxes, r.rays)
            assert (ot > 0).sum() > 20
            out = g.trace_ex(r.rays, want=("t", "prim", "normal"))
            assert np.array_equal(out["t"].view(np.uint32), ot.view(np.uint32)) and np.array_equal(out["prim"], op), name
            assert np.array_equal(out["normal"], oracle.cube_normals(r.boxes, op, r.rays, ot)), name + ": normal"
            assert np.array_equal(g.trace_ex(r.rays, want=("t",))["t"].view(np.uint32), ot.view(np.uint32))
            sh = g.trace_ex(r.rays, any_hit=True, want=("shadowed",))["shadowed"]
            assert np.array_equal(sh, oracle.trace_any_brute(r.boxes, r.rays)), name + ": shadowed"
            tpr = np.random.default_rng(3).uniform(0.0, 0.6 * float(ot.max()), len(r.rays)).astype(F)
            sh = g.trace_ex(r.rays, tmax_per_ray=tpr, any_hit=True, want=("shadowed",))["shadowed"]
            assert np.array_equal(sh, oracle.trace_any_brute(r.boxes, r.rays, tmax_per_ray=tpr)) and 0 < sh.sum() < len(r.rays)
            # the compacted hit list, on the device
            n = len(r.rays)
            dr = torch.from_numpy(np.array(r.rays)).cuda()
            dt = torch.empty(n, dtype=torch.float32, device="cuda")
            dp = torch.empty(n, dtype=torch.int32, device="cuda")
            dh = torch.zeros(n * 3, dtype=torch.int32, device="cuda")
            dn = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            g.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr(), dh.data_ptr(), dn.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(dt.cpu().numpy(), ot) and np.array_equal(dp.cpu().numpy().view(np.uint32), op)
            nh = int(dn.cpu().item())
            idx = np.flatnonzero(ot > 0)
            assert nh == len(idx)
            hits = np.sort(dh.cpu().numpy().view(gpu.HIT)[:nh], order=("ray",))
            assert np.array_equal(hits["ray"], idx) and np.array_equal(hits["prim"], op[idx]) and np.array_equal(hits["t"], ot[idx])
            # rays generated in the kernel: the rule of test_gpu_parity (the same hit pattern, t within 1e-5 of the restated rays' brute force)
            hi = np.asarray(sc.ORG) + np.asarray(r.dims) * float(sc.VS)
            cam = camera(eye=tuple(hi + (0.7 * hi[0], 0.5 * hi[0], -0.9 * hi[0])), ctr=tuple((np.asarray(sc.ORG) + hi) / 2))
            ct = g.trace_ex(camera=cam, want=("t", "prim", "normal"))
            crays = oracle.primary_rays(cam[0], cam[1], W, H)
            rt, rp = oracle.trace_brute(r.boxes, crays)
            assert (rt > 0).sum() >= 10
            assert np.array_equal(ct["t"] > 0, rt > 0) and np.allclose(ct["t"], rt, rtol=0, atol=1e-5), name + ": camera rays"
            same = ct["prim"] == rp
            assert same.mean() > 0.999 and np.array_equal(ct["normal"][same], oracle.cube_normals(r.boxes, rp, crays, rt)[same])
        # a Vec list still pending beside a device batch
        s = soup_ref(sc.LARGE)
        rays = soup_rays(sc.LARGE)
        ot, op = oracle.trace_brute(s.boxes, rays)
        mesh = gpu.Mesh.from_arrays(s.v, s.t)
        g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, gpu.GRID_VEC)
        g.revoxelize(mesh, sc.SOUP_VS, list_async=True)
        dr = torch.from_numpy(np.array(rays)).cuda()                 # (a writable copy: the shared rays are read-only)
        dt = torch.empty(len(rays), dtype=torch.float32, device="cuda")
        dp = torch.empty(len(rays), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.trace_device(dr.data_ptr(), len(rays), dt.data_ptr(), dp.data_ptr())
        g.list_wait()
        torch.cuda.synchronize()
        assert np.array_equal(dt.cpu().numpy(), ot) and np.array_equal(dp.cpu().numpy().view(np.uint32), op)
        assert g.aabbs().tobytes() == s.vec.tobytes()


# ---- 5. ordered hits on the grid -----------------------------------------------------------------------------------------------------------
def cursor_after(got, at, ap):
    n = len(at)
    last = np.maximum((got["t"] > 0).sum(axis=1) - 1, 0)
    have = got["t"][:, 0] > 0
    return (np.where(have, got["t"][np.arange(n), last], at).astype(F), np.where(have, got["prim"][np.arange(n), last], ap).astype(np.uint32))


@patterns
def test_trace_multi(gpu, pattern):
    with poisoned(gpu, pattern):
        for name in ("large_half", "small_tenth", "small_full"):
            r = mask_ref(name)
            g = sc.masked_grid(gpu, r.cells)
            cnt = mr.select(r.times, 1)[2]
            if name == "large_half":
                assert (cnt > 32).any()                                     # counts above K = 32
            assert (cnt > 1).any() and (cnt == 0).any()
            for k in (32, 1):
                ref = mr.select(r.times, k)
                same_hits(g.trace_multi(r.rays, max_hits=k), ref, "%s K=%d" % (name, k))
                same_hits(g.trace_multi(r.rays, max_hits=k, want=("t", "prim")), ref, "%s K=%d, no count" % (name, k))
                same_hits(g.trace_multi(r.rays, max_hits=k, want=("count",)), ref, "%s K=%d, count only" % (name, k))
            n = len(r.rays)
            cur = (np.full(n, F(-1), F), np.full(n, 12345, np.uint32))       # (-1, anything) = no cursor
            for page in range(3):
                got = g.trace_multi(r.rays, max_hits=5, after=cur)
                same_hits(got, mr.select(r.times, 5, after=cur), "%s page %d" % (name, page))
                cur = cursor_after(got, *cur)
            one = g.trace_ex(r.rays, want=("t", "prim"))
            ref = mr.select(r.times, 1)
            assert np.array_equal(one["t"].view(np.uint32), ref[0][:, 0].view(np.uint32))


# ---- 6. the octree's rays ------------------------------------------------------------------------------------------------------------------
@patterns
def test_octree_trace(gpu, pattern):
    with poisoned(gpu, pattern):
        for dims in (sc.LARGE, sc.SMALL):
            s = soup_ref(dims)
            rays = soup_rays(dims)
            mesh = gpu.Mesh.from_arrays(s.v, s.t)
            ref = octree_ref(dims, 16)
            boxes, items = ref["aabbs"], ref["items"]
            ot, op = oracle.trace_brute(boxes, rays)
            times = om.hit_times(boxes, items, rays)
            tpr = np.random.default_rng(4).uniform(0.0, 0.6 * float(ot.max()), len(rays)).astype(F)
            for max_items in (16, 1, 100):
                o = gpu.Octree(mesh, sc.SOUP_VS, max_items)
                what = "%s max_items %d" % (dims, max_items)
                out = o.trace_ex(rays, want=("t", "prim", "normal"))
                assert np.array_equal(out["t"].view(np.uint32), ot.view(np.uint32)) and np.array_equal(out["prim"], op), what
                assert np.array_equal(out["normal"], oracle.cube_normals(boxes, op, rays, ot)), what + ": normal"
                sh = o.trace_ex(rays, tmax_per_ray=tpr, any_hit=True, want=("shadowed",))["shadowed"]
                assert np.array_equal(sh, oracle.trace_any_brute(boxes, rays, tmax_per_ray=tpr)), what + ": shadowed"
                for k in (32, 1):
                    same_hits(o.trace_multi(rays, max_hits=k), mr.select(times, k), "%s K=%d" % (what, k))
                n = len(rays)
                cur = (np.full(n, F(-1), F), np.full(n, 12345, np.uint32))
                for page in range(2):
                    got = o.trace_multi(rays, max_hits=3, after=cur)
                    same_hits(got, mr.select(times, 3, after=cur), "%s page %d" % (what, page))
                    cur = cursor_after(got, *cur)


# ---- 7. the triangle BVH -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sliver_ref():
    c = sc.sliver_case()
    r = Ref()
    r.closest = mesh_ref.closest(c.v, c.t, c.rays)
    r.tpr = np.random.default_rng(5).uniform(0.0, 4.0, len(c.rays)).astype(F)
    r.any = mesh_ref.any_hit(c.v, c.t, c.rays, tmax_per_ray=r.tpr)
    with np.errstate(all="ignore"):
        r.normals = mesh_ref.normals(c.v, c.t, r.closest[1])
    r.normal_ok = np.isfinite(r.normals).all(axis=1)                                 # (a collinear triangle has no normal to compare)
    return r


@patterns
def test_bvh(gpu, pattern):
    with poisoned(gpu, pattern):
        c = sc.sliver_case()
        r = sliver_ref()
        mesh = gpu.Mesh.from_arrays(c.v, c.t)
        for max_leaf in (0, 1):
            b = mesh.bvh(max_leaf=max_leaf)
            what = "max_leaf %d" % max_leaf
            assert b.num_ill_conditioned == int(mc.side_listed(c.v, c.t).sum()) > 50
            assert np.array_equal(np.sort(b.leaf_triangles()), np.arange(len(c.t)))
            check_closest(b, c.v, c.t, c.rays, what, r.closest)
            out = b.trace_ex(c.rays, want=("t", "normal", "bary"))
            assert np.abs(out["normal"] - r.normals)[r.normal_ok].max() <= 1e-6         # the tolerance of test_gpu_mesh_trace
            miss = r.closest[1] == mesh_ref.MISS
            assert not out["normal"][miss].any() and not out["bary"][miss].any()
            sh = b.trace_ex(c.rays, tmax_per_ray=r.tpr, any_hit=True, want=("shadowed",))["shadowed"]
            assert np.array_equal(sh, r.any) and 0 < sh.sum() < len(c.rays)
            for k in (32, 1):
                ref = mm.select(c.hits, k)
                same_mesh_hits(b.trace_multi(c.rays, max_hits=k, want=ALL), ref, "%s K=%d" % (what, k))
                same_mesh_hits(b.trace_multi(c.rays, max_hits=k, want=("t", "prim", "bary")), ref, "%s K=%d, no count" % (what, k))
            cur = None
            for page in range(2):
                got = b.trace_multi(c.rays, max_hits=3, after=cur, want=ALL)
                same_mesh_hits(got, mm.select(c.hits, 3, after=cur), "%s page %d" % (what, page))
                cur = mm.cursor_of(got, cur)
        # a radix tree that is a chain (a ray holds one stack entry per level), mirrored and not
        for mirrored in (False, True):
            ch = dt.chain_scene(64, mirrored)
            rays = dt.deep_rays(64, mirrored)
            b = gpu.Mesh.from_arrays(ch.v, ch.t).bvh(max_leaf=1)
            assert b.height == dt.radix_height(dt.bvh_keys(ch.v, ch.t))
            check_closest(b, ch.v, ch.t, rays, ch.name, dt.chain_closest(64, mirrored))
            same_mesh_hits(b.trace_multi(rays, max_hits=32, want=ALL), mm.select(dt.chain_hits(64, mirrored), 32), ch.name + " K=32")


# ---- 8. instances --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tlas_updates():
    """the multi-hit case's instances (one masked out), then two more sets of the same count: one with a singular and a degenerate
    transform and another masked instance, one shuffled"""
    c = mc.tlas_case()
    a = c.inst.copy()
    b = c.inst.copy()
    b["transform"][0] = instance_ref.transform(scale=(0, 1, 1))
    b["transform"][5] = instance_ref.transform(scale=(1, 0, 0))
    b["mask"][1], b["mask"][3] = 0, 0xFF
    d = c.inst[::-1].copy()
    return a, b, d


@patterns
def test_tlas(gpu, pattern):
    import torch
    with poisoned(gpu, pattern):
        c = mc.tlas_case()
        rays = c.rays[::3]
        a, b, d = tlas_updates()
        bl = [gpu.Mesh.from_arrays(v, t).bvh() for v, t in c.meshes]
        tl = gpu.Tlas(bl, a)
        tlas_check(tl, c.meshes, a, rays, "build")
        for k in (32, 1):
            same_mesh_hits(tl.trace_multi(c.rays, max_hits=k, want=ALL_TLAS), mm.select(c.hits, k), "K=%d" % k)
        tpr = np.random.default_rng(6).uniform(0.0, 12.0, len(rays)).astype(F)
        sh = tl.trace_ex(rays, tmax_per_ray=tpr, any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(sh, instance_ref.any_hit(c.meshes, a, rays, tmax_per_ray=tpr))
        tl.update(b)
        tlas_check(tl, c.meshes, b, rays, "update: singular and masked instances")
        same_mesh_hits(tl.trace_multi(rays, max_hits=4, want=ALL_TLAS), mm.select(mm.all_hits_tlas(c.meshes, b, rays), 4), "after the update")
        dev = torch.from_numpy(d.view(np.uint8).copy()).to("cuda")
        tl.update(device_ptr=dev, count=len(d))
        tlas_check(tl, c.meshes, d, rays, "update from a device array")
        w, _ = instance_ref.inverse(d["transform"])
        assert np.array_equal(tl.world_to_object().view(np.uint32), w.view(np.uint32))
        tl.update(a)
        same_mesh_hits(tl.trace_multi(c.rays, max_hits=2, want=ALL_TLAS), mm.select(c.hits, 2), "back to the first instances")
        pc = dt.pure_chain_instances(8)                               # every split isolates one instance: height n - 1
        ptl = gpu.Tlas([gpu.Mesh.from_arrays(v, t).bvh() for v, t in pc.meshes], pc.inst)
        assert ptl.height() == 7
        tlas_check(ptl, pc.meshes, pc.inst, pc.rays, "a chain of instances")


# ---- 9. frames -----------------------------------------------------------------------------------------------------------------------------
@patterns
def test_frames(gpu, pattern, tmp_path):
    with poisoned(gpu, pattern):
        v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
        mesh = gpu.Mesh.from_arrays(v, t)
        vs = F(0.05)
        cam = camera((6.16636, 2.42256, -3.15471), (0.0, 1.0, 0.0))
        vi, pi = cam[0], cam[1]
        # a grid and a BVH
        write_mesh_obj(str(tmp_path / "scene.obj"), True)
        model = gpu.Mesh.load_obj(str(tmp_path / "scene.obj"))
        mv, mtris = model.host_arrays()
        mats, ids = model.materials()
        vox, bvh = gpu.Grid.voxelize(mesh, vs), model.bvh()
        ref = frame_reference(vox, W, H, vi, pi, bvh, (mv, mtris, mats, ids))
        assert (ref["kind"] == 1).sum() > 50 and (ref["kind"] == 2).sum() > 50 and ref["shadowed"].sum() > 5
        r = gpu.Renderer(vox, bvh, model)
        check_frame(r, ref, cam, what="grid + BVH")
        r.free()
        # an octree alone
        oct_ = gpu.Octree(mesh, vs)
        ref = frame_reference(oct_, W, H, vi, pi)
        assert (ref["kind"] == 1).sum() > 50
        r = gpu.Renderer(oct_)
        check_frame(r, ref, cam, what="octree")
        r.free()
        # instances, beside voxels
        meshes, blas, tl, inst, host, imats = instanced_scene(gpu, tmp_path)
        bv, bt = vx_scenes.cube(half=0.75, center=(0.0, 3.5, 0.0))
        ivox = gpu.Grid.voxelize(gpu.Mesh.from_arrays(bv, bt), vs)
        icam = camera((7.0, 5.0, -8.0), (0.0, 0.5, 0.0))
        ref = inst_reference(ivox, tl, host, imats, inst, icam)
        assert (ref["kind"] == 2).sum() > 100 and (ref["kind"] == 1).sum() > 5
        r = gpu.Renderer.from_tlas(ivox, tl, meshes)
        inst_check(r, ref, icam, "TLAS")
        r.free()
        # attribute shading with a texture
        obj, img = write_textured_plane(tmp_path)
        plane = gpu.Mesh.load_obj(str(obj))
        plane.load_textures()
        pb = plane.bvh()
        bv, bt = vx_scenes.cube(half=0.4, center=(0.0, 1.5, 0.0))
        pvox = gpu.Grid.voxelize(gpu.Mesh.from_arrays(bv, bt), vs)
        pcam = camera((0.5, 5.0, -4.0), (0.0, 0.0, 0.0))
        r = gpu.Renderer(pvox, pb, plane, attributes=True)
        ref = attr_bvh_reference(pvox, pb, plane, pcam, render_ref.DEFAULT_LIGHT)
        out = attr_check(r, ref, pcam, None, "textured plane")
        assert (out["kind"] == 2).sum() > 500
        r.free()


# ---- 10. solid fill ------------------------------------------------------------------------------------------------------------------------
@patterns
def test_solid(gpu, pattern):
    with poisoned(gpu, pattern):
        for kind in kinds(gpu):
            for cells in (sc.cavity_cells(), sc.mask("small_tenth"), sc.mask("large_half")):
                g = sc.masked_grid(gpu, cells, kind)
                sc.check_fill(gpu, g, cells, "kind %d" % kind)
        for name, vs in (("rotcube", 0.09), ("torus", 0.05)):
            v, t = solid_scene(name)
            mesh = gpu.Mesh.from_arrays(v, t)
            exp = solid_expected(v, t, F(vs), 0)
            assert exp[5] > 0
            for kind in kinds(gpu):
                check_solid(gpu, gpu.Grid.voxelize(mesh, F(vs), kind, solid=True), kind, v, t, F(vs), 0, exp)


# ---- 11 to 15. the analysis of a mask ------------------------------------------------------------------------------------------------------
MASKS = [name for name, _ in sc.mask_cases()]


@patterns
def test_distance(gpu, pattern):
    with poisoned(gpu, pattern):
        for name in MASKS:
            sc.check_distance(sc.masked_grid(gpu, sc.mask(name)), sc.mask(name))


@patterns
def test_nearest(gpu, pattern):
    with poisoned(gpu, pattern):
        for name in MASKS:
            sc.check_nearest(sc.masked_grid(gpu, sc.mask(name)), sc.mask(name))


@patterns
def test_morph(gpu, pattern):
    with poisoned(gpu, pattern):
        bit, dist = sc.morph_radii(gpu)
        assert np.sqrt(bit) <= gpu.morph_bit_radius() < np.sqrt(dist)
        for name in MASKS:
            for kind in (kinds(gpu) if name == "small_tenth" else (gpu.GRID_BOOL,)):
                sc.check_morph(gpu, sc.masked_grid(gpu, sc.mask(name), kind), sc.mask(name), what="%s kind %d" % (name, kind))
        sparse = sc.sparse_cells(sc.LARGE, 5)                       # large balls that grow and leave something to erode
        sc.check_morph(gpu, sc.masked_grid(gpu, sparse), sparse, what="sparse")
        sc.check_morph(gpu, sc.masked_grid(gpu, ~sparse), ~sparse, what="sparse holes")


@patterns
def test_surfaces(gpu, pattern):
    with poisoned(gpu, pattern):
        for name in MASKS:
            sc.check_surfaces(gpu, sc.masked_grid(gpu, sc.mask(name)), sc.mask(name))
        for dims in (sc.LARGE, sc.SMALL):                            # with per-cell material ids
            r = soup_ref(dims)
            mesh = gpu.Mesh.from_arrays(r.v, r.t)
            mesh.set_materials(*sc.material_records(gpu, len(r.t)))
            for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT):
                g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, kind, materials=True)
                assert len(np.unique(g.materials()[1])) > 1
                sc.check_surfaces(gpu, g, r.cells, materials=True)


@patterns
def test_components(gpu, pattern):
    with poisoned(gpu, pattern):
        for name in MASKS:
            sc.check_components(sc.masked_grid(gpu, sc.mask(name)), sc.mask(name))
        sparse = sc.random_cells(sc.LARGE, 0.12, 21)                # many parts
        sc.check_components(sc.masked_grid(gpu, sparse), sparse)


# ---- 16. the sort and the scan -------------------------------------------------------------------------------------------------------------
@patterns
def test_sort_and_scan(gpu, pattern):
    with poisoned(gpu, pattern):
        rng = np.random.default_rng(pattern & 0xFFFF)
        for bits in (9, 33, 64):
            hi = (1 << bits) - 1
            for n in (1, 65, 4097, 39271):
                k = rng.integers(0, hi, n, dtype=np.uint64, endpoint=True)
                k[rng.integers(0, n, n // 3)] = k[0]
                assert np.array_equal(gpu.sort_u64(k, bits), np.sort(k)), (bits, n)
        for n in (0, 17, sr.TILE - 1, 2 * sr.TILE + 6502):           # the last: the cells of the large grid
            x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            for mode in ("values", "popcount"):
                caps = dict(sel_cap=(32 * n) // 1024 + 16) if mode == "popcount" else {}
                for path in ("gen", "ticket", "three"):
                    r = gpu.scan_u32([x], mode=mode, paths=path, total_tag=TAG, group16_cap=n // 16 + 17, **caps)[0]
                    assert r["taken"] == expect_path(path, n)
                    scan_check(r, x, mode, path, "%s n=%d [%s]" % (mode, n, path), group16_cap=n // 16 + 17, **caps)
            y = rng.integers(0, 256, n, dtype=np.uint8)
            for path in ("gen", "ticket"):
                for ioff, ooff in ((0, 0), (3, 1)):
                    r = gpu.scan_u32([y], mode="bytes", paths=path, in_offset=ioff, out_offset=ooff, total_tag=TAG)[0]
                    scan_check(r, y, "bytes", path, "bytes n=%d [%s] offsets %d/%d" % (n, path, ioff, ooff))
        # scans of shrinking and growing sizes on one scratch block, the three paths interleaved
        sizes = [40000, 17, 0, 2 * sr.TILE + 1, 5, 16385]
        paths = ["gen", "ticket", "gen", "three", "gen", "ticket"]
        xs = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in sizes]
        for k, (x, p, r) in enumerate(zip(xs, paths, gpu.scan_u32(xs, paths=paths, total_tag=TAG))):
            scan_check(r, x, "values", p, "scan %d of the sequence" % k)
