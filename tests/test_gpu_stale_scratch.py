"""A handle's own leftovers.  Every handle keeps its scratch blocks from call to call, sized by the largest call so far: after a large, dense
call a small, sparse and differently shaped one works in blocks that still hold the large call's words (and its flags, counters and scan
state), and the large call that follows finds the small one's.  On ONE handle each: large, small, large again; one mode of a feature
after another at fixed dimensions; ray batches of 4096, 1, 4096 rays; K = 32 then K = 1; a cursor, then none; rebuilds of a BVH and updates
of a TLAS to fewer primitives and back; frames of 64 x 48, 3 x 1, 64 x 48 pixels.  Every step is compared with its reference
(tests/*_ref.py, oracle.py), never with an earlier step.  Shapes and the checks of the grid analysis: tests/stale_cases.py."""
import functools

import numpy as np
import pytest

import components_ref as cr
import distance_ref as dr
import instance_ref
import mesh_multihit_cases as mc
import mesh_multihit_ref as mm
import mesh_ref
import morph_ref as mor
import multihit_ref as mr
import nearest_ref as nr
import nets_ref
import octree_multihit_ref as om
import oracle
import solid_ref
import stale_cases as sc
import surface_ref as sr
import vx_scenes
from test_gpu_instances import check as tlas_check, random_transforms
from test_gpu_mesh_multihit import ALL, ALL_TLAS, same as same_mesh_hits
from test_gpu_mesh_trace import check_closest, write_mesh_obj
from test_gpu_multihit import same as same_hits
from test_gpu_nets import same as same_arrays
from test_gpu_render import check_frame, reference as frame_reference

pytestmark = pytest.mark.gpu

F = np.float32
STEPS = ((sc.LARGE, 1), (sc.SMALL, 1), (sc.LARGE, 2))      # (dimensions, seed of the soup): large and dense, small and sparse, large again


# ---- the grid analysis, all three flavours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["bool", "aabbstruct", "vec"])
def test_grid_analysis_large_small_large(gpu, kind):
    mat = kind != gpu.GRID_VEC                                # per-cell ids (the surfaces' materials): one id per cell only without Vec
    g = None
    for step, (dims, seed) in enumerate(STEPS):
        r = sc.soup_ref(dims, 0, seed)
        what = "step %d %s" % (step, dims)
        mesh = gpu.Mesh.from_arrays(r.v, r.t)
        recs, ids = sc.material_records(gpu, len(r.t))
        mesh.set_materials(recs, ids)
        if g is None:
            g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, kind, materials=mat)
        else:
            g.revoxelize(mesh, sc.SOUP_VS, materials=mat)
        sc.check_build(gpu, g, kind, r, what)
        if mat:
            sc.check_material_ids(gpu, g, kind, r, recs, ids)
        filled = sc.check_analysis(gpu, g, r.cells, materials=mat, what=what)
        # the filled grid is a mask like any other: once more round the features that read the most scratch
        sc.check_distance(g, filled, device=False)
        sc.check_components(g, filled, device=False)


# ---- one handle's scan scratch across the generation / ticket boundary -------------------------------------------------------------------------
POP8 = np.array([bin(b).count("1") for b in range(256)], np.uint8)


def test_scan_scratch_across_the_ticket_boundary(gpu):
    """The single-pass scan numbers its scans on a scratch block up to 512 tiles of 16384 elements (8 388 608) and hands out tickets, on
    cleared status words, above: a Bool grid of 1024 x 1024 x 257 cells (8 421 376 mask words) lies just above it, one of 128 x 128 x 33 far below.
    One handle: large, small, large, small -- every word-prefix scan after the first finds the other mode's status words.  The reference
    is numpy's popcount of the mask, which no scan has touched."""
    v, t = vx_scenes.cube(half=0.5, center=(0.5, 0.5, 0.5))
    mesh = gpu.Mesh.from_arrays(v * F([1024, 1024, 257]), t)
    assert len(t) == 12
    g, tris = None, []
    for step, (vs, dim) in enumerate(((1.0, (1024, 1024, 257)), (8.0, (128, 128, 33))) * 2):
        if g is None:
            g = gpu.Grid.voxelize(mesh, vs, gpu.GRID_BOOL)
        else:
            g.revoxelize(mesh, vs)
        d = g.describe()
        assert d["dim"] == dim, step
        if dim[0] == 1024:
            assert d["num_words"] == 8421376 > 512 * 16384
        occupied = int(POP8[g.bitmask().view(np.uint8)].sum(dtype=np.int64))
        assert occupied > 0 and d["occupied"] == occupied, "step %d: %d occupied, the mask holds %d" % (step, d["occupied"], occupied)
        assert len(g.aabbs()) == occupied, step
        if dim[0] == 1024:                                         # two scans of different length on the one block
            tris.append(g.surface_counts()[1])
    assert tris[0] > 0 and tris[0] == tris[1]


# ---- one mode after another at fixed dimensions ----------------------------------------------------------------------------------------------
def test_distance_modes_then_nearest(gpu):
    cells = sc.mask("large_half")
    g = sc.masked_grid(gpu, cells)
    d_out, d_in = dr.edt_sq_c(cells), dr.edt_sq_c(~cells)
    s = dr.sdf_from(cells, d_out, d_in, sc.VS)
    n_out, n_in = nr.nearest_c(cells), nr.nearest_c(~cells)
    for rep in range(2):
        assert np.array_equal(g.distance_sq(), d_out), "outside, round %d" % rep
        assert np.array_equal(g.distance_sq(inside=True), d_in), "inside, round %d" % rep
        assert g.sdf().tobytes() == s.tobytes(), "sdf, round %d" % rep                # (both envelopes: the stack block grows)
        assert np.array_equal(g.nearest(), n_out), "nearest after the fields, round %d" % rep
        assert np.array_equal(g.distance_sq(inside=True), d_in), "inside after nearest, round %d" % rep
        assert np.array_equal(g.nearest(inside=True), n_in)
        vals = np.random.default_rng(rep).integers(0, 1 << 32, cells.size, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(g.nearest_gather(vals, fill=7), nr.gather(n_out, vals, 7))
        assert np.array_equal(g.distance_sq(), d_out)
    # the same handle with a sparse mask: most cells far from every target
    sparse = sc.sparse_cells(sc.LARGE, 5)
    sc.write_cells(gpu, g, sparse)
    sc.check_distance(g, sparse, device=False)
    sc.check_nearest(g, sparse, device=False)


def test_morph_paths_and_operations(gpu):
    bit, dist = sc.morph_radii(gpu)
    for cells in (sc.mask("large_half"), sc.sparse_cells(sc.LARGE, 5), ~sc.sparse_cells(sc.LARGE, 6)):
        g = sc.masked_grid(gpu, cells)
        want = {(op, r2): sc.words_of(mor.apply_fast(op, cells, r2, c=True)) for op in (mor.DILATE, mor.ERODE, mor.OPEN, mor.CLOSE) for r2 in (bit, dist)}
        order = [(mor.CLOSE, dist), (mor.ERODE, bit), (mor.CLOSE, bit), (mor.ERODE, dist), (mor.OPEN, dist), (mor.DILATE, bit), (mor.OPEN, bit),
                 (mor.DILATE, dist), (mor.CLOSE, dist), (mor.ERODE, dist)]
        for k, (op, r2) in enumerate(order):
            got = g.morph_mask(op, r2)
            assert np.array_equal(got, want[(op, r2)]), "call %d: op %d r2=%d, %d words differ" % (k, op, r2, int((got != want[(op, r2)]).sum()))
        sc.check_mask(g, cells, "the source mask")


def test_components_connectivities_then_stats(gpu):
    for cells in (sc.random_cells(sc.LARGE, 0.12, 21), sc.mask("large_half")):
        g = sc.masked_grid(gpu, cells)
        ref = {c: cr.label(cells, c) for c in (6, 26)}
        assert ref[6][1] > ref[26][1] >= 1
        for c in (26, 6, 26):
            lab, k = g.components(c)
            assert k == ref[c][1] and np.array_equal(lab, ref[c][0]), "connectivity %d" % c
        for c in (6, 26, 6):                                       # the statistics label again: more parts, then fewer, then more
            s = g.component_stats(c)
            assert s.tobytes() == cr.stats(*ref[c]).tobytes(), "stats, connectivity %d" % c
        lab, k = g.components(26)
        assert k == ref[26][1] and np.array_equal(lab, ref[26][0])


def test_smooth_surface_then_plain(gpu):
    r = sc.soup_ref(sc.LARGE)
    mesh = gpu.Mesh.from_arrays(r.v, r.t)
    mesh.set_materials(*sc.material_records(gpu, len(r.t)))
    g = gpu.Grid.voxelize(mesh, sc.SOUP_VS, gpu.GRID_BOOL, materials=True)
    d = g.describe()
    cell_ids = g.materials()[1]
    smooth = nets_ref.surface_smooth(r.cells, d["origin"], F(d["voxel_size"]), 3, 0.5, -0.53, cell_ids=cell_ids, with_normals=True)
    plain = sr.surface(r.cells, d["origin"], F(d["voxel_size"]))
    with_ids = sr.surface(r.cells, d["origin"], F(d["voxel_size"]), cell_ids=cell_ids)
    for rep in range(2):
        same_arrays(g.surface_smooth(3, 0.5, -0.53, materials=True, normals=True), smooth, "smooth, round %d" % rep)
        same_arrays(g.surface(), plain, "plain, round %d" % rep)
        same_arrays(g.surface(materials=True), with_ids, "with ids, round %d" % rep)
        same_arrays(g.surface_smooth(3, 0.5, -0.53), smooth[:2], "smooth without extras, round %d" % rep)
    # then a small surface in the same blocks
    small = sc.soup_ref(sc.SMALL)
    ms = gpu.Mesh.from_arrays(small.v, small.t)
    g.revoxelize(ms, sc.SOUP_VS)
    d = g.describe()
    same_arrays(g.surface_smooth(3, 0.5, -0.53, normals=True),
                nets_ref.surface_smooth(small.cells, d["origin"], F(d["voxel_size"]), 3, 0.5, -0.53, with_normals=True), "small, smooth")
    same_arrays(g.surface(), sr.surface(small.cells, d["origin"], F(d["voxel_size"])), "small, plain")


@pytest.mark.parametrize("kind", [0, 2], ids=["bool", "vec"])
def test_fill_interior_cavity_closed_then_opened(gpu, kind):
    closed, opened = sc.cavity_cells(), sc.cavity_cells(opened=True)
    g = sc.masked_grid(gpu, closed, kind)
    sc.check_fill(gpu, g, closed, "closed")
    rounds_closed = g.fill_rounds()
    sc.write_cells(gpu, g, opened)                                 # the whole mask again, one wall cell missing
    sc.check_mask(g, opened, "opened")
    if kind == gpu.GRID_BOOL:
        filled = sc.check_fill(gpu, g, opened, "opened")
        assert int(filled.sum()) < int(solid_ref.unpack(solid_ref.fill(sc.words_of(closed), sc.LARGE)[0], sc.LARGE).sum())
    else:                                                          # (a Vec list keeps the records of the first fill: the mask and the count here)
        sw, hw, nh = solid_ref.fill(sc.words_of(opened), sc.LARGE)
        assert g.fill_interior() == nh and np.array_equal(g.bitmask(), sw)
    assert g.fill_rounds() >= 1 and rounds_closed >= 1
    sc.write_cells(gpu, g, closed)                                 # and closed again
    sw, hw, nh = solid_ref.fill(sc.words_of(closed), sc.LARGE)
    assert g.fill_interior() == nh and np.array_equal(g.bitmask(), sw)


# ---- ray batches of 4096, 1 and 4096 rays; K = 32 then 1; a cursor, then none ----------------------------------------------------------------
BATCHES = (4096, 1, 4096)


def first_hits(h, rays, idx, ref, what, fields=("t", "prim")):
    out = h.trace_ex(rays[idx], want=fields)
    for f in fields:
        a, b = out[f], ref[f][idx]
        if f != "normal":                                          # (bit for bit; the cube normals by value, as their own tests compare them)
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s: %s differs on %d rays" % (what, f, int((a != b).reshape(len(a), -1).any(1).sum()))


def multi_switches(h, rays, select, same, want, what):
    """K = 32, K = 1, K = 32; a page behind a cursor, then the first page again"""
    for k in (32, 1, 32):
        same(h.trace_multi(rays, max_hits=k, want=want), select(k, None), "%s K=%d" % (what, k))
    first = h.trace_multi(rays, max_hits=3, want=want)
    same(first, select(3, None), what + " first page")
    return first


def test_grid_ray_batches(gpu):
    for name in ("large_half", "small_tenth"):
        r = sc.mask_ref(name)
        ot, op = oracle.trace_brute(r.boxes, r.rays)
        ref = dict(t=ot, prim=op, normal=oracle.cube_normals(r.boxes, op, r.rays, ot))
        g = sc.masked_grid(gpu, r.cells)
        for n in BATCHES:
            first_hits(g, r.rays, sc.tiled(len(r.rays), n), ref, "%s %d rays" % (name, n), ("t", "prim", "normal"))
        for n in BATCHES:                                          # prim alone: the ray kernel's own rank epilogue and its ring
            first_hits(g, r.rays, sc.tiled(len(r.rays), n), ref, "%s %d rays, prim" % (name, n), ("prim",))
        for n in BATCHES:
            idx = sc.tiled(len(r.rays), n)
            tt, pp, nh = g.trace(r.rays[idx])
            assert np.array_equal(tt, ot[idx]) and np.array_equal(pp, op[idx]) and nh == int((ot[idx] > 0).sum())
        sel = lambda k, after: mr.select(r.times, k, after=after)
        first = multi_switches(g, r.rays, sel, same_hits, ("t", "prim", "count"), name)
        n = len(r.rays)
        last = np.maximum((first["t"] > 0).sum(axis=1) - 1, 0)
        have = first["t"][:, 0] > 0
        cur = (np.where(have, first["t"][np.arange(n), last], F(-1)).astype(F), np.where(have, first["prim"][np.arange(n), last], 0).astype(np.uint32))
        same_hits(g.trace_multi(r.rays, max_hits=3, after=cur), mr.select(r.times, 3, after=cur), name + " second page")
        same_hits(g.trace_multi(r.rays, max_hits=3), mr.select(r.times, 3), name + " without the cursor")
        same_hits(g.trace_multi(r.rays[:1], max_hits=32), tuple(a[:1] for a in mr.select(r.times, 32)), name + " one ray")


def test_octree_ray_batches(gpu):
    s = sc.soup_ref(sc.LARGE)
    rays = sc.soup_rays(sc.LARGE)
    ref = oracle.octree(s.v, s.t, sc.SOUP_VS, max_items=16, threads=2)
    boxes, items = ref["aabbs"], ref["items"]
    ot, op = oracle.trace_brute(boxes, rays)
    fh = dict(t=ot, prim=op, normal=oracle.cube_normals(boxes, op, rays, ot))
    times = om.hit_times(boxes, items, rays)
    for max_items in (16, 100):
        o = gpu.Octree(gpu.Mesh.from_arrays(s.v, s.t), sc.SOUP_VS, max_items)
        for n in BATCHES:
            first_hits(o, rays, sc.tiled(len(rays), n), fh, "max_items %d, %d rays" % (max_items, n), ("t", "prim", "normal"))
        sel = lambda k, after: mr.select(times, k, after=after)
        first = multi_switches(o, rays, sel, same_hits, ("t", "prim", "count"), "max_items %d" % max_items)
        n = len(rays)
        last = np.maximum((first["t"] > 0).sum(axis=1) - 1, 0)
        have = first["t"][:, 0] > 0
        cur = (np.where(have, first["t"][np.arange(n), last], F(-1)).astype(F), np.where(have, first["prim"][np.arange(n), last], 0).astype(np.uint32))
        same_hits(o.trace_multi(rays, max_hits=3, after=cur), mr.select(times, 3, after=cur), "second page")
        same_hits(o.trace_multi(rays, max_hits=3), mr.select(times, 3), "without the cursor")


@functools.lru_cache(maxsize=None)
def sliver_first_hits():
    c = sc.sliver_case()
    t, p, b = mesh_ref.closest(c.v, c.t, c.rays)
    return dict(t=t, prim=p, bary=b)


def three_triangles():
    v = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [2, 2, 2], [3, 2, 2], [2, 3, 2.5]])
    return v, np.arange(9, dtype=np.int32).reshape(3, 3)


def test_bvh_ray_batches_and_rebuilds(gpu):
    c = sc.sliver_case()
    ref = sliver_first_hits()
    mesh = gpu.Mesh.from_arrays(c.v, c.t)
    b = mesh.bvh()
    for n in BATCHES:
        first_hits(b, c.rays, sc.tiled(len(c.rays), n), ref, "%d rays" % n, ("t", "prim", "bary"))
    sel = lambda k, after: mm.select(c.hits, k, after=after)
    first = multi_switches(b, c.rays, sel, same_mesh_hits, ALL, "slivers")
    cur = mm.cursor_of(first, None)
    same_mesh_hits(b.trace_multi(c.rays, max_hits=3, after=cur, want=ALL), mm.select(c.hits, 3, after=cur), "second page")
    same_mesh_hits(b.trace_multi(c.rays, max_hits=3, want=ALL), mm.select(c.hits, 3), "without the cursor")
    # build_into: about 2000 triangles -> 3 -> back
    v3, t3 = three_triangles()
    m3 = gpu.Mesh.from_arrays(v3, t3)
    r3 = vx_scenes.random_rays(500, F([-1, -1, -1]), F([4, 4, 4]), seed=31)
    hits3 = mm.all_hits(v3, t3, r3)
    for rep in range(2):
        b.build_into(m3)
        assert b.num_triangles == 3 and b.num_ill_conditioned == 0 and np.array_equal(np.sort(b.leaf_triangles()), np.arange(3))
        check_closest(b, v3, t3, r3, "three triangles, round %d" % rep)
        same_mesh_hits(b.trace_multi(r3, max_hits=2, want=ALL), mm.select(hits3, 2), "three triangles, K=2")
        b.build_into(mesh)
        assert b.num_triangles == len(c.t) and b.num_ill_conditioned == int(mc.side_listed(c.v, c.t).sum())
        assert np.array_equal(np.sort(b.leaf_triangles()), np.arange(len(c.t)))
        check_closest(b, c.v, c.t, c.rays, "back, round %d" % rep, (ref["t"], ref["prim"], ref["bary"]))
        same_mesh_hits(b.trace_multi(c.rays, max_hits=4, want=ALL), mm.select(c.hits, 4), "back, K=4")


def test_tlas_ray_batches_and_updates(gpu):
    import torch
    c = mc.tlas_case()
    bl = [gpu.Mesh.from_arrays(v, t).bvh() for v, t in c.meshes]
    tl = gpu.Tlas(bl, c.inst)
    t, i, p, b = instance_ref.closest(c.meshes, c.inst, c.rays)
    ref = dict(t=t, instance=i, prim=p, bary=b)
    for n in BATCHES:
        first_hits(tl, c.rays, sc.tiled(len(c.rays), n), ref, "%d rays" % n, ("t", "instance", "prim", "bary"))
    sel = lambda k, after: mm.select(c.hits, k, after=after)
    first = multi_switches(tl, c.rays, sel, same_mesh_hits, ALL_TLAS, "six instances")
    cur = mm.cursor_of(first, None, tlas=True)
    same_mesh_hits(tl.trace_multi(c.rays, max_hits=3, after=cur, want=ALL_TLAS), mm.select(c.hits, 3, after=cur), "second page")
    same_mesh_hits(tl.trace_multi(c.rays, max_hits=3, want=ALL_TLAS), mm.select(c.hits, 3), "without the cursor")
    # updates: 64 instances -> 1 -> 0 -> 64
    rays = c.rays[::4]
    many = [instance_ref.make_instances(random_transforms(64, seed=s, spread=4.0), blas=[k % 2 for k in range(64)]) for s in (3, 4)]
    one = instance_ref.make_instances([instance_ref.transform(offset=(0.5, 0.0, 0.3))], blas=[1])
    none = instance_ref.make_instances([], blas=[])
    for step, inst in enumerate((many[0], one, none, many[1], one, many[0])):
        if step == 3:                                              # (once from a device array)
            dev = torch.from_numpy(inst.view(np.uint8).copy()).to("cuda")
            tl.update(device_ptr=dev, count=len(inst))
        else:
            tl.update(inst)
        assert tl.num_instances() == len(inst) and tl.num_nodes() == max(2 * len(inst) - 1, 0)
        what = "step %d: %d instances" % (step, len(inst))
        if len(inst):
            tlas_check(tl, c.meshes, inst, rays, what)
            same_mesh_hits(tl.trace_multi(rays, max_hits=4, want=ALL_TLAS), mm.select(mm.all_hits_tlas(c.meshes, inst, rays), 4), what)
        else:
            tt, ii, pp, nh = tl.trace(rays)
            assert nh == 0 and (tt == -1).all() and (ii == 0xFFFFFFFF).all() and (pp == 0xFFFFFFFF).all(), what
            assert not tl.trace_multi(rays, max_hits=4, want=("count",))["count"].any()


# ---- frames of 64 x 48, 3 x 1 and 64 x 48 pixels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["grid", "octree"])
def test_frame_sizes(gpu, tmp_path, source):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    mesh = gpu.Mesh.from_arrays(v, t)
    vs = F(0.05)
    write_mesh_obj(str(tmp_path / "scene.obj"), True)
    model = gpu.Mesh.load_obj(str(tmp_path / "scene.obj"))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    vox = gpu.Grid.voxelize(mesh, vs) if source == "grid" else gpu.Octree(mesh, vs)
    bvh = model.bvh()
    r = gpu.Renderer(vox, bvh, model)
    for W, H in ((64, 48), (3, 1), (64, 48), (1, 1), (64, 48)):
        vi, pi = vx_scenes.camera_matrices(aspect=W / H)
        ref = frame_reference(vox, W, H, vi, pi, bvh, (mv, mtris, mats, ids))
        if W == 64:
            assert (ref["kind"] == 1).sum() > 50 and (ref["kind"] == 2).sum() > 50
        check_frame(r, ref, (vi, pi, W, H), what="%s %dx%d" % (source, W, H))
    r.free()
