"""The device-memory pool stays balanced: every block a handle or a call takes goes back when the handle is freed or the call returns
(vx_device_live_blocks), after a build that fails as well; a Vec grid's list survives every move into a larger block; a handle that
changes its stream builds what a fresh handle builds."""
import gc

import numpy as np
import pytest

import instance_ref
import vx_scenes

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(0.12)                          # the rotated cube at 28^3 cells or so
ERR_MORTON_BITS, ERR_CAPACITY = 5, 8
TINY = F(1e-7)                        # the cube at 3e7 cells per axis: above 2^21


def live(gpu):
    return gpu.device_live_blocks()


def settled(gpu):
    """the count once the handles that other tests dropped without free() are gone -- now, not halfway through a measurement"""
    gc.collect()
    return live(gpu)


def balanced(gpu, cycle):
    """create -> use -> free leaves the pool where it was (after one warm-up cycle)"""
    cycle()
    before = settled(gpu)
    cycle()
    assert live(gpu) == before


def twice(gpu, call):
    """the second of two identical calls leaves the pool where the first left it: staging blocks go back, handle scratch stays"""
    call()
    first = live(gpu)
    out = call()
    assert live(gpu) == first
    return out


def cube_rays(n=64):
    v, _ = vx_scenes.rotated_cube()
    return vx_scenes.random_rays(n, v.min(0) - F(0.5), v.max(0) + F(0.5), seed=3)


def camera(w=8, h=8):
    vi, pi = vx_scenes.camera_matrices(eye=(4.0, 3.0, -5.0), ctr=(0.0, 0.0, 0.0), aspect=w / h)
    return vi, pi, w, h


def four_instances():
    return [instance_ref.transform(offset=(3.0 * k, 0.0, 0.0)) for k in range(4)]


def test_mesh_balanced(gpu):
    v, t = vx_scenes.rotated_cube()

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        g = gpu.Grid.voxelize(m, VS, materials=False)   # (uploads the mesh)
        g.free()
        m.free()
    balanced(gpu, cycle)


@pytest.mark.parametrize("kind", ["GRID_BOOL", "GRID_AABBSTRUCT", "GRID_VEC"])
def test_grid_balanced(gpu, kind):
    kind = getattr(gpu, kind)
    v, t = vx_scenes.rotated_cube()
    rays = cube_rays()

    def use(g):
        twice(gpu, lambda: g.trace(rays))
        twice(gpu, lambda: g.trace_ex(rays, want=("t", "prim", "normal")))
        twice(gpu, lambda: g.trace_ex(rays, any_hit=True, tmax_per_ray=np.full(len(rays), 50.0, F), want=("shadowed",)))
        twice(gpu, lambda: g.trace_multi(rays, max_hits=4))
        twice(gpu, g.aabbs)
        twice(gpu, g.distance_sq)
        twice(gpu, g.sdf)
        twice(gpu, g.surface)
        twice(gpu, lambda: g.surface_mesh().free())
        twice(gpu, g.components)
        twice(gpu, g.component_stats)

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        g = gpu.Grid.voxelize(m, VS, kind)
        use(g)
        g.revoxelize(m, F(0.2))
        use(g)
        g.revoxelize(m, VS)
        assert g.fill_interior() > 0
        use(g)
        g.free()
        c = gpu.Grid.create(kind, 8, 8, 8, F(0.5), origin=(-2.0, -2.0, -2.0))
        for p in ((1, 1, 1), (6, 5, 4), (7, 7, 7)):
            c.set_voxel(*p)
        use(c)
        assert c.fill_interior() == 0
        c.free()
        m.free()
    balanced(gpu, cycle)


def test_octree_balanced(gpu):
    v, t = vx_scenes.rotated_cube()
    rays = cube_rays()

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        for max_items in (16, 1 << 20):               # the direct node build and the level-by-level one
            o = gpu.Octree(m, VS, max_items=max_items)
            assert o.num_items > 0
            twice(gpu, lambda: o.trace(rays))
            twice(gpu, lambda: o.trace_ex(rays, want=("t", "prim", "normal")))
            twice(gpu, o.aabbs)
            o.free()
        m.free()
    balanced(gpu, cycle)


def test_octree_node_array_is_a_pool_block(gpu):
    """the node array is one more live block whichever form builds it -- the direct one (16), the level-by-level one (65, and 1 << 20: the
    lone root) -- and free() returns every block"""
    v, t = vx_scenes.rotated_cube()
    m = gpu.Mesh.from_arrays(v, t)
    gpu.Octree(m, VS).free()                          # (uploads the mesh)
    rises = []
    for max_items in (16, 65, 1 << 20):
        before = settled(gpu)
        o = gpu.Octree(m, VS, max_items=max_items)
        assert o.num_nodes > 0
        rises.append(live(gpu) - before)
        o.free()
        assert live(gpu) == before
    assert rises[0] == rises[1] == rises[2] and rises[0] > 0, rises
    m.free()


def test_bvh_tlas_renderer_balanced(gpu):
    v, t = vx_scenes.rotated_cube()
    rays = cube_rays()
    cam = camera()

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        b = gpu.Bvh(m)
        twice(gpu, lambda: b.trace(rays))
        twice(gpu, lambda: b.trace_ex(rays, want=("t", "prim", "bary", "normal")))
        b.build_into(m)
        twice(gpu, lambda: b.trace(rays))
        tl = gpu.Tlas([b], gpu.instances(four_instances()))
        twice(gpu, lambda: tl.trace(rays))
        twice(gpu, lambda: tl.trace_ex(rays))
        tl.update(gpu.instances(four_instances()[::-1]))
        twice(gpu, lambda: tl.trace(rays))
        g = gpu.Grid.voxelize(m, VS)
        o = gpu.Octree(m, VS)
        for vox in (g, o):
            r = gpu.Renderer(vox, b, m)
            twice(gpu, lambda: r.render_host(cam, want=("rgba", "kind", "shadowed")))
            r.free()
            r = gpu.Renderer.from_tlas(vox, tl, [m])
            twice(gpu, lambda: r.render_host(cam, want=("rgba", "kind", "shadowed")))
            r.free()
        r = gpu.Renderer.from_tlas(None, tl, [m], attributes=True)
        twice(gpu, lambda: r.render_host(cam))
        r.free()
        for h in (o, g, tl, b, m):
            h.free()
    balanced(gpu, cycle)


def test_multi_sort_scan_balanced(gpu):
    v, t = vx_scenes.rotated_cube()
    keys = np.random.default_rng(1).integers(0, 1 << 40, 1000, dtype=np.uint64)
    words = np.random.default_rng(2).integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        mu = gpu.Multi(m, [0])
        for _ in range(2):
            g = mu.voxelize(VS)[0]
            assert g.describe()["occupied"] > 0
        mu.free()
        mu = gpu.Multi(m, [0, 0])                     # two logical ranks on one device: shards and their exchange
        mu.voxelize(VS, materials=False)
        mu.free()
        m.free()
        assert np.array_equal(twice(gpu, lambda: gpu.sort_u64(keys, 40)), np.sort(keys))
        r = twice(gpu, lambda: gpu.scan_u32([words, words[:100]], mode="popcount", paths=["gen", "three"]))
        assert r[0]["total"] & ((1 << 48) - 1) == int(np.unpackbits(words.view(np.uint8)).sum())
    balanced(gpu, cycle)


def test_failed_builds_leave_nothing_behind(gpu):
    """builds that return an error status after their scratch exists, without any HIP error: the octree above 2^21 cells per axis (its
    scratch and mailbox are local to the build), and vx_voxelize_into / vx_voxelize above them (the handle keeps its blocks; a fresh
    handle is deleted)"""
    v, t = vx_scenes.rotated_cube()
    m = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(m, VS, gpu.GRID_VEC)
    gpu.Octree(m, VS).free()
    before = settled(gpu)
    for _ in range(2):
        with pytest.raises(gpu.VxError) as ei:
            gpu.Octree(m, TINY)
        assert ei.value.status == ERR_MORTON_BITS
        assert live(gpu) == before
        with pytest.raises(gpu.VxError) as ei:
            g.revoxelize(m, TINY)
        assert ei.value.status == ERR_CAPACITY
        assert live(gpu) == before
        with pytest.raises(gpu.VxError) as ei:
            gpu.Grid.voxelize(m, TINY, gpu.GRID_VEC)
        assert ei.value.status == ERR_CAPACITY
        assert live(gpu) == before
        g.revoxelize(m, VS)                           # the handle builds again, in the blocks it kept
        assert live(gpu) == before
    g.free()
    m.free()


# ---------------------------------------------------------------------------------------------- Vec list growth
def cell_aabbs(gpu, cells, vs, origin):
    """cell_aabb (vx_math.h) in float32: c = org + (i + 0.5) * vs per axis, {c - vs / 2, c + vs / 2}"""
    c = F(origin)[None, :] + (np.asarray(cells, F) + F(0.5)) * F(vs)
    half = F(vs) * F(0.5)
    out = np.zeros(len(cells), dtype=gpu.AABB)
    out["mn"], out["mx"] = c - half, c + half
    return out


def test_vec_list_growth_by_set_voxel(gpu):
    """24 bytes per record: the list moves to a larger block at the 1st, 11th and 43rd record (blocks of 256, 1024 and 4096 bytes)"""
    vs, org = F(0.25), (0.5, -1.0, 2.0)
    rng = np.random.default_rng(9)
    cells = [tuple(int(x) for x in rng.integers(0, 4, 3)) for _ in range(44)]   # (the same cell twice appends twice)

    def cycle():
        g = gpu.Grid.create(gpu.GRID_VEC, 4, 4, 4, vs, origin=org)
        for k, c in enumerate(cells):
            g.set_voxel(*c)
            assert g.aabbs().tobytes() == cell_aabbs(gpu, cells[:k + 1], vs, org).tobytes(), k
        assert g.describe()["set_calls"] == len(cells) and g.memory_bytes() == 24 * len(cells)
        g.free()
    balanced(gpu, cycle)


def diagonal_triangles(n=6):
    """n small triangles, triangle k strictly inside cell (k, k, k) of the grid of voxel size 1 they span (origin 0): a Vec build's
    list is cell (k, k, k) once, in this order"""
    v, t = [], []
    for k in range(n):
        o = 0.0 if k == 0 else k + 0.4                # (triangle 0 puts the bounding box's corner, the grid's origin, at 0)
        v += [(o, o, o), (o + 0.2, o, o + 0.1), (o, o + 0.2, o + 0.1)]
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.array(v, F), np.array(t, np.int32)


def test_vec_list_leaves_the_bound_buffer(gpu):
    """a list a build left in the caller's buffer (8 records) continues in the grid's own storage from the first append on, the earlier
    records intact -- there and in the caller's buffer"""
    import torch
    v, t = diagonal_triangles()
    first = [(k, k, k) for k in range(6)]
    rng = np.random.default_rng(10)
    more = [tuple(int(x) for x in rng.integers(0, 6, 3)) for _ in range(20)]    # the own block of 512 bytes is outgrown at the 22nd record

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        buf = torch.full((8 * 6,), -7.0, dtype=torch.float32, device="cuda")
        g = gpu.Grid.create(gpu.GRID_VEC, 1, 1, 1, F(1.0))
        g.bind_aabbs_device(buf.data_ptr(), 8)
        g.revoxelize(m, F(1.0))
        assert g.describe()["dim"] == (6, 6, 6)
        exp = cell_aabbs(gpu, first, 1.0, (0.0, 0.0, 0.0))
        assert g.aabbs().tobytes() == exp.tobytes()
        torch.cuda.synchronize()
        assert buf.cpu().numpy()[:36].tobytes() == exp.tobytes()                # the build wrote the caller's buffer
        for k, c in enumerate(more):
            g.set_voxel(*c)
            assert g.aabbs().tobytes() == cell_aabbs(gpu, first + more[:k + 1], 1.0, (0.0, 0.0, 0.0)).tobytes(), k
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert host[:36].tobytes() == exp.tobytes() and (host[36:] == -7.0).all(), k   # appends go to the grid's own storage
        g.free()
        m.free()
    balanced(gpu, cycle)


def test_vec_list_growth_by_fill_interior(gpu):
    """a hollow 6^3 shell set cell by cell (152 records), then its 4^3 interior in ascending cell order behind them.  (A bound buffer
    of 8 records cannot hold a closed shell, so this path has no bound variant.)"""
    vs, org = F(0.5), (-1.0, 0.0, 1.0)
    shell = [(x, y, z) for z in range(6) for y in range(6) for x in range(6) if 0 in (x, y, z) or 5 in (x, y, z)]
    inner = [(x, y, z) for z in range(1, 5) for y in range(1, 5) for x in range(1, 5)]

    def cycle():
        g = gpu.Grid.create(gpu.GRID_VEC, 6, 6, 6, vs, origin=org)
        for c in shell:
            g.set_voxel(*c)
        assert g.aabbs().tobytes() == cell_aabbs(gpu, shell, vs, org).tobytes()
        assert g.fill_interior() == len(inner)
        assert g.aabbs().tobytes() == cell_aabbs(gpu, shell + inner, vs, org).tobytes()
        assert g.fill_interior() == 0                                           # nothing left to fill: the list stays
        assert g.aabbs().tobytes() == cell_aabbs(gpu, shell + inner, vs, org).tobytes()
        g.set_voxel(0, 0, 0)
        assert g.aabbs().tobytes() == cell_aabbs(gpu, shell + inner + [(0, 0, 0)], vs, org).tobytes()
        d = g.describe()
        assert d["occupied"] == 216 and d["set_calls"] == len(shell) + len(inner) + 1
        g.free()
    balanced(gpu, cycle)


@pytest.mark.parametrize("kind", ["GRID_BOOL", "GRID_VEC"])
def test_stream_switch(gpu, kind):
    """a handle built on one stream and rebuilt on another gives a fresh build's bitmask and list, and all its blocks go back"""
    import torch
    kind = getattr(gpu, kind)
    v, t = vx_scenes.rotated_cube()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def cycle():
        m = gpu.Mesh.from_arrays(v, t)
        fresh = gpu.Grid.voxelize(m, VS, kind)
        g = gpu.Grid.voxelize(m, F(0.2), kind, stream=s1.cuda_stream)
        g.aabbs()
        g.revoxelize(m, VS, stream=s2.cuda_stream)
        assert np.array_equal(g.bitmask(), fresh.bitmask())
        assert g.aabbs().tobytes() == fresh.aabbs().tobytes() and len(fresh.aabbs()) > 0
        g.revoxelize(m, VS, stream=s1.cuda_stream)      # and back, at the sizes the blocks already have
        assert np.array_equal(g.bitmask(), fresh.bitmask())
        assert g.aabbs().tobytes() == fresh.aabbs().tobytes()
        for h in (g, fresh, m):
            h.free()
    balanced(gpu, cycle)
