"""The voxelizer at its documented limits and after failed rebuilds.

- Grids of exactly 2^21 cells on one axis (include/voxhip.h: "at most 2^21 cells per axis", inclusive): triangles that span the whole
  axis, 2^21 - 1 cells, 2^16 cells and start at cell 65536, on x, y and z, against the CPU oracle bit for bit -- Bool (both SAT
  variants), AABBstruct, Vec (also VX_VOXELIZE_LIST_ASYNC), per-voxel materials, Octree, word shards and rays.
- vx_voxelize_into's failure contract (voxhip.h): an error the arguments alone show leaves the previous build untouched, every other
  error leaves an empty grid, and the next build on the handle equals a fresh handle's.
- The two spare words behind the bitmask stay zero when a handle is rebuilt at a smaller grid, tiled or direct.
- The 2^32 edges: a unit total past 2^32, occupied counts and primitive ids next to 2^32, frames of 2^32 pixels, and the bits past
  the last cell of an externally written mask.
"""
import numpy as np
import pytest

import oracle
import vx_scenes

pytestmark = pytest.mark.gpu

AXIS_MAX = 1 << 21
THREADS = 16        # oracle threads
TMAX = 4.0e6        # rays cross a whole 2^21-cell axis
ERR_INVALID_ARG, ERR_OUT_OF_BOUNDS, ERR_MORTON_BITS, ERR_CAPACITY = 1, 4, 5, 8


def long_axis_mesh(axis, ncells, nsmall=3000, spanning=True, seed=21):
    """A mesh ncells x 4 x 4 cells of size 1, the long side on `axis` (0, 1, 2).  The bounding box is pinned to [0, ncells] x [0, 4] x
    [0, 4], so vs = 1 gives exactly ncells cells (every coordinate is exact in float32).  Slim triangles run along the long axis over
    cells [0, n), [1, n), [0, n - 1), [65536, n) and exactly 2^16 cells; `nsmall` small ones are scattered along it.  The long ones are
    spread through the index range so that the oracle's threads share them."""
    L = float(ncells)
    rng = np.random.default_rng(seed + 7 * axis + ncells % 97)
    c = np.stack([rng.uniform(0.0, L, nsmall), rng.uniform(0.5, 3.5, nsmall), rng.uniform(0.5, 3.5, nsmall)], 1)
    tri = c[:, None, :] + rng.uniform(-1.4, 1.4, (nsmall, 3, 3))
    tri[:, :, 0] = np.clip(tri[:, :, 0], 0.0, L)
    tri[:, :, 1:] = np.clip(tri[:, :, 1:], 0.0, 4.0)
    tri[0, 0] = (0.5 * L, 0.0, 0.0)                 # pin the thin sides of the box
    tri[1, 0] = (0.25 * L, 4.0, 4.0)
    if spanning:
        long_ = np.array([[[0.0, 1.3, 1.6], [L, 2.6, 2.2], [0.5 * L, 2.2, 2.7]],                     # cells [0, n): crosses rows too
                          [[1.25, 1.2, 1.3], [L, 1.7, 1.4], [0.625 * L, 1.5, 1.75]],                # [1, n)
                          [[0.0, 1.25, 1.4], [L - 1.25, 1.8, 1.6], [0.375 * L, 1.4, 1.7]],          # [0, n - 1)
                          [[65536.25, 2.2, 1.2], [L, 2.7, 1.8], [0.75 * L, 2.4, 1.5]],              # [65536, n)
                          [[1000.25, 1.2, 2.2], [66535.75, 1.8, 2.7], [30000.5, 1.4, 2.4]]])        # [1000, 1000 + 2^16)
        step = len(tri) // len(long_)
        for k, lt in enumerate(long_):
            tri = np.insert(tri, k * step + step // 2, lt, axis=0)
    else:
        tri[2, 0, 0], tri[3, 0, 0] = 0.0, L         # the long side of the box
    perm = {0: (0, 1, 2), 1: (1, 0, 2), 2: (1, 2, 0)}[axis]   # column of the (long, a, b) coordinate that goes to x, y, z
    tri = tri[:, :, perm].astype(np.float32)
    v = np.ascontiguousarray(tri.reshape(-1, 3))
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, t


def long_axis_rays(axis, ncells, seed):
    """Rays along the long axis from both ends (the far end's first hits are spanning triangles' voxels near cell 2^21 - 1), steep rays
    across the thin sides around cells 0, 65536 and n - 1 and everywhere, and random rays from outside."""
    L = float(ncells)
    rng = np.random.default_rng(seed)
    rows = []
    m = 160
    ab = np.concatenate([rng.uniform(1.3, 2.6, (m // 2, 2)), rng.uniform(0.05, 3.95, (m - m // 2, 2))])   # half in the long triangles' rows
    rows.append(np.concatenate([np.full((m, 1), L + 9.0), ab, np.full((m, 1), -1.0), rng.uniform(-2e-6, 2e-6, (m, 2))], 1))
    rows.append(np.concatenate([np.full((m, 1), -9.0), ab, np.full((m, 1), 1.0), rng.uniform(-2e-6, 2e-6, (m, 2))], 1))
    for centre in (0.0, 65536.0, L - 1.0, None):
        p = rng.uniform(0.0, L, m) if centre is None else np.clip(centre + rng.uniform(-40.0, 40.0, m), 0.0, L)
        o = np.stack([p, np.full(m, -3.0), rng.uniform(-1.0, 5.0, m)], 1)
        tgt = np.stack([p + rng.uniform(-2.0, 2.0, m), rng.uniform(0.0, 4.0, m), rng.uniform(0.0, 4.0, m)], 1)
        rows.append(np.concatenate([o, tgt - o], 1))
    o = np.stack([rng.uniform(-100.0, L + 100.0, m), rng.uniform(-30.0, 34.0, m), rng.uniform(-30.0, 34.0, m)], 1)
    tgt = np.stack([rng.uniform(0.0, L, m), rng.uniform(0.0, 4.0, m), rng.uniform(0.0, 4.0, m)], 1)
    rows.append(np.concatenate([o, tgt - o], 1))
    r = np.concatenate(rows)
    perm = {0: [0, 1, 2], 1: [1, 0, 2], 2: [1, 2, 0]}[axis]
    r = r[:, perm + [3 + k for k in perm]]
    return np.ascontiguousarray(r, dtype=np.float32)


def _materials(nt):
    recs = np.zeros(5, dtype=[("ambient", np.float32, 3), ("diffuse", np.float32, 3), ("specular", np.float32, 3), ("transmittance", np.float32, 3),
                              ("emission", np.float32, 3), ("shininess", np.float32), ("ior", np.float32), ("dissolve", np.float32),
                              ("illum", np.int32), ("texture_id", np.int32)])
    recs["diffuse"][:, 0] = np.arange(5) / 8.0      # five distinct values, none equal to MaterialObj{}
    recs["texture_id"] = -1
    ids = (np.arange(nt) % 6 - 1).astype(np.int32)  # -1: no material
    tv = np.where(ids >= 0, ids + 1, 0).astype(np.int32)   # value ids: 0 = MaterialObj{}, then the records in order
    return recs, ids, tv, 6


CASES = [(0, AXIS_MAX), (1, AXIS_MAX), (2, AXIS_MAX), (0, AXIS_MAX - 1), (1, AXIS_MAX - 1), (2, AXIS_MAX - 1), (0, AXIS_MAX - 31)]


@pytest.mark.parametrize("axis,ncells", CASES, ids=["%s%d" % ("xyz"[a], n) for a, n in CASES])
def test_axis_limit_parity(gpu, axis, ncells):
    """Exactly 2^21 (and 2^21 - 1, and on x 2^21 - 31: the direct, untiled mask) cells on one axis, triangles over the whole axis: every
    grid flavour, the Octree, word shards by rank and rays bit-equal to the oracle."""
    v, t = long_axis_mesh(axis, ncells)
    vs = np.float32(1.0)
    mesh = gpu.Mesh.from_arrays(v, t)
    dim = [4, 4, 4]
    dim[axis] = ncells
    for sat in (0, 1):
        ow, calls, gi = oracle.build_bool(v, t, vs, threads=THREADS, sat=sat)
        assert gi["dim"] == tuple(dim)
        g = gpu.Grid.voxelize(mesh, vs, gpu.GRID_BOOL, sat_variant=sat)
        d = g.describe()
        assert d["dim"] == gi["dim"] and d["set_calls"] == calls
        w = g.bitmask()
        assert np.array_equal(w, ow), "sat %d: %d differing words" % (sat, int((w != ow).sum()))
        if sat == 0:
            oa = oracle.bool_aabbs(ow, gi, vs)
            assert g.aabbs().tobytes() == oa.tobytes() and d["occupied"] == len(oa)
            ow0, g0 = ow, g
        else:
            assert g.aabbs().tobytes() == oracle.bool_aabbs(ow, gi, vs).tobytes()
        del g
    ow, g, gi = ow0, g0, oracle.grid_info(v, vs)
    oa = oracle.bool_aabbs(ow, gi, vs)
    assert (oa["mn"][:, axis] == np.float32(ncells - 1)).sum() >= 2     # the long triangles reach the last cell of the axis
    # AABBstruct
    ga = gpu.Grid.voxelize(mesh, vs, gpu.GRID_AABBSTRUCT)
    oab, by = oracle.build_aabbstruct(v, t, vs, threads=THREADS, sat=0)
    assert ga.memory_bytes() == by and ga.aabbs().tobytes() == oab.tobytes()
    del ga, oab
    # Vec, in call order -- directly and with the list left to its first reader
    ov = oracle.build_vec(v, t, vs, threads=THREADS, sat=0)
    gv = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)
    assert gv.aabbs().tobytes() == ov.tobytes()
    gv.revoxelize(mesh, vs, list_async=True)
    assert gv.memory_bytes() == 24 * len(ov) and gv.aabbs().tobytes() == ov.tobytes()
    del gv, ov
    # per-voxel material ids (k_mat_last decodes the same ranges)
    recs, ids, tv, nvalues = _materials(len(t))
    mm = gpu.Mesh.from_arrays(v, t)
    mm.set_materials(recs, ids)
    gm = gpu.Grid.voxelize(mm, vs, gpu.GRID_BOOL, materials=True)
    oids, order = oracle.material_ids(v, t, vs, tv, nvalues)
    assert np.array_equal(gm.bitmask(), ow)
    mats, mid = gm.materials()
    assert np.array_equal(mid, oids) and len(mats) == len(order)
    del gm, mm, oids
    # Octree (2^21 cells per axis is the reference's own bound, inclusive)
    o = gpu.Octree(mesh, vs)
    r = oracle.octree(v, t, vs, threads=THREADS)
    assert np.array_equal(o.items(), r["items"]) and o.nodes().tobytes() == r["nodes"].tobytes()
    assert o.aabbs().tobytes() == r["aabbs"].tobytes() and o.memory_bytes() == r["bytes"]
    del o, r
    # word shards by rank (a long z axis: the z-slab path of the record kernel)
    nw = len(ow)
    for world in (2, 4):
        acc = np.zeros_like(ow)
        for rank in range(world):
            wb, we, _ = gpu.shard_words(nw, rank, world)
            ws = gpu.Grid.voxelize(mesh, vs, shard=(rank, world)).bitmask()
            assert not ws[:wb].any() and not ws[we:].any() and np.array_equal(ws[wb:we], ow[wb:we]), (rank, world)
            acc |= ws
        assert np.array_equal(acc, ow)
    # rays: the walk on all of them, the brute force over every box on a share
    rays = long_axis_rays(axis, ncells, seed=axis * 7 + ncells % 13)
    tt, pp, _ = g.trace(rays, tmax=TMAX)
    wt, wp = oracle.trace_walk(ow, gi, vs, rays, tmax=TMAX, threads=THREADS)
    assert np.array_equal(tt, wt) and np.array_equal(pp, wp)
    assert (wt > 0).sum() > 200
    far_hits = wp[:160][wt[:160] > 0]                    # rays from the far end: first hits near cell n - 1
    assert (oa["mn"][far_hits.astype(np.int64), axis] > ncells - 64).sum() >= 20
    sub = rays[::4]
    bt, bp = oracle.trace_brute(oa, sub, tmax=TMAX, threads=THREADS)
    assert np.array_equal(tt[::4], bt) and np.array_equal(pp[::4], bp)
    ex = g.trace_ex(sub, tmax=TMAX, want=("t", "prim", "normal"))
    assert np.array_equal(ex["t"], bt) and np.array_equal(ex["prim"], bp)
    assert np.array_equal(ex["normal"], oracle.cube_normals(oa, bp, sub, bt))


def test_axis_limit_errors(gpu):
    """2^21 cells on an axis are accepted by the grid and the Octree; 2^21 + 1 are not: VX_ERR_CAPACITY for the grid, the reference's
    VX_ERR_MORTON_BITS message for the Octree."""
    v, t = long_axis_mesh(0, AXIS_MAX, nsmall=2000, spanning=False)
    mesh = gpu.Mesh.from_arrays(v, t)
    vs = np.float32(1.0)
    ow, _, gi = oracle.build_bool(v, t, vs, threads=THREADS, sat=0)
    assert gi["dim"] == (AXIS_MAX, 4, 4)
    g = gpu.Grid.voxelize(mesh, vs)
    assert g.describe()["dim"] == gi["dim"] and np.array_equal(g.bitmask(), ow)
    o = gpu.Octree(mesh, vs)
    assert np.array_equal(o.items(), oracle.octree(v, t, vs, threads=THREADS)["items"])
    over = np.float32(AXIS_MAX / (AXIS_MAX + 0.5))
    assert oracle.grid_info(v, over)["dim"][0] == AXIS_MAX + 1
    with pytest.raises(gpu.VxError) as ei:
        gpu.Grid.voxelize(mesh, over)
    assert ei.value.status == ERR_CAPACITY
    with pytest.raises(gpu.VxError) as ei:
        gpu.Octree(mesh, over)
    assert ei.value.status == ERR_MORTON_BITS
    assert ei.value.message == "We support up to 21 bits per axis (max 2^21 voxels per dimension)!"


# ---------------------------------------------------------------------------------------------- failed rebuilds
FLAVOURS = {  # name: (kind, revoxelize flags, bound caller buffer)
    "bool": ("GRID_BOOL", {}, False),
    "aabbstruct": ("GRID_AABBSTRUCT", {}, False),
    "vec": ("GRID_VEC", {}, False),
    "vec_async": ("GRID_VEC", {"list_async": True}, False),
    "vec_bound": ("GRID_VEC", {}, True),
    "bool_materials": ("GRID_BOOL", {"materials": True}, False),
}


def _scene_a():
    v, t = vx_scenes.scene("soup2000")
    return v, t, np.float32(0.02)


def _read(gpu, g, rays, probes, cap):
    """Everything a caller can read from a grid."""
    import torch
    d = g.describe()
    w = g.bitmask()
    assert len(w) == d["num_words"] == (int(np.prod(d["dim"])) + 31) // 32     # dims and mask always agree
    out = dict(dim=d["dim"], occupied=d["occupied"], set_calls=d["set_calls"], triangles=d["triangles"], words=w.tobytes(),
               bytes=g.memory_bytes(), aabbs=g.aabbs().tobytes())
    buf = torch.full((cap * 6,), -7.0, dtype=torch.float32, device="cuda")
    n = g.aabbs_device(buf.data_ptr(), cap)
    torch.cuda.synchronize()
    out["aabbs_device"] = (n, buf.cpu().numpy()[: min(n, cap) * 6].tobytes())
    vox = []
    for p in probes:
        try:
            vox.append(g.test_voxel(*p))
        except gpu.VxError as e:
            vox.append(("error", e.status))
    out["test_voxel"] = vox
    tt, pp, nh = g.trace(rays)
    out["trace"] = (tt.tobytes(), pp.tobytes(), nh)
    ex = g.trace_ex(rays, want=("t", "prim", "normal"))
    out["trace_ex"] = (ex["t"].tobytes(), ex["prim"].tobytes(), ex["normal"].tobytes())
    mats, mid = g.materials()
    out["materials"] = (mats.tobytes(), mid.tobytes())
    return out


def _assert_empty(gpu, r, nrays, nprobes):
    assert r["dim"] == (0, 0, 0) and r["words"] == b"" and r["occupied"] == 0 and r["set_calls"] == 0 and r["triangles"] == 0
    assert r["aabbs"] == b"" and r["aabbs_device"] == (0, b"") and r["bytes"] == 0
    assert r["test_voxel"] == [("error", ERR_OUT_OF_BOUNDS)] * nprobes
    t = np.frombuffer(r["trace"][0], np.float32)
    assert len(t) == nrays and not (t > 0).any() and r["trace"][2] == 0
    assert not (np.frombuffer(r["trace_ex"][0], np.float32) > 0).any() and not np.frombuffer(r["trace_ex"][2], np.float32).any()
    assert r["materials"] == (b"", b"")


def _assert_same(a, b, what):
    for k in a:
        assert a[k] == b[k], "%s: %s differs" % (what, k)


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_failed_rebuild_leaves_defined_state(gpu, flavour):
    """vx_voxelize_into's failure contract (voxhip.h), through every reader: an error the arguments alone show leaves build A as it was
    (a VX_VOXELIZE_LIST_ASYNC list that was never read included); every later error -- an axis above 2^21 cells, more than 2^37 cells,
    a word range past the new grid's words on a reused and on a fresh block -- leaves the empty grid; and rebuilding A on the handle
    gives what a fresh handle gives."""
    import torch
    kind_name, flags, bound = FLAVOURS[flavour]
    kind = getattr(gpu, kind_name)
    v, t, vs = _scene_a()
    mesh = gpu.Mesh.from_arrays(v, t)
    if flags.get("materials"):
        recs, ids, _, _ = _materials(len(t))
        mesh.set_materials(recs, ids)
    gi = oracle.grid_info(v, vs)
    rays = vx_scenes.random_rays(3000, gi["bmin"], gi["bmin"] + np.array(gi["dim"], np.float32) * vs, seed=31)
    ow = oracle.build_bool(v, t, vs)[0]
    rng = np.random.default_rng(5)
    occ = np.flatnonzero(np.unpackbits(ow.view(np.uint8), bitorder="little"))
    X, Y, _ = gi["dim"]
    probes = [tuple(int(rng.integers(0, n)) for n in gi["dim"]) for _ in range(16)]
    probes += [(int(i % X), int(i // X % Y), int(i // (X * Y))) for i in rng.choice(occ, 8, replace=False)]
    ref = gpu.Grid.voxelize(mesh, vs, kind, materials=flags.get("materials", False))
    cap = ref.describe()["set_calls"] + 64
    exp = _read(gpu, ref, rays, probes, cap)
    assert exp["words"] == ow.tobytes() and sum(x is True for x in exp["test_voxel"]) >= 8

    # failures -- (name, revoxelize arguments, status, leaves A)
    ext = np.array(gi["bmax"], np.float64) - np.array(gi["bmin"], np.float64)
    vs_axis = np.float32(ext.max() / (AXIS_MAX + 4096.0))
    vs_cells = np.float32(ext.min() / 6000.0)
    dc = oracle.grid_info(v, vs_cells)["dim"]
    assert max(dc) <= AXIS_MAX and int(np.prod(dc, dtype=np.float64)) > (1 << 37)
    nw = len(ow)
    vs_big = np.float32(vs * 0.5)
    nw_big = (int(np.prod(oracle.grid_info(v, vs_big)["dim"])) + 31) // 32
    # the same geometry with a material table the int16 ids cannot index: MaterialObj{} + 32767 distinct records
    many = gpu.Mesh.from_arrays(v, t)
    recs_many = np.zeros(32767, dtype=_materials(1)[0].dtype)
    recs_many["diffuse"][:, 0] = np.arange(32767) + 2.0
    recs_many["texture_id"] = -1
    many.set_materials(recs_many, (np.arange(len(t)) % 32767).astype(np.int32))
    failures = [("sat_variant", dict(voxel_size=vs, sat_variant=2), ERR_INVALID_ARG, True),
                ("material_table", dict(voxel_size=vs, mesh=many, materials=True), ERR_CAPACITY, True),
                ("shard_rank", dict(voxel_size=vs, shard=(2, 2)), ERR_INVALID_ARG, True),
                ("tris", dict(voxel_size=vs, tris=(0, len(t) + 1)), ERR_INVALID_ARG, True),
                ("axis_above_2^21", dict(voxel_size=vs_axis), ERR_CAPACITY, False),
                ("above_2^37_cells", dict(voxel_size=vs_cells), ERR_CAPACITY, False),
                ("words_past_end_reused", dict(voxel_size=vs, words=(0, nw + 1)), ERR_INVALID_ARG, False),
                ("words_past_end_fresh", dict(voxel_size=vs_big, words=(0, nw_big + 1)), ERR_INVALID_ARG, False)]

    g = gpu.Grid.voxelize(mesh, vs, kind, materials=flags.get("materials", False))
    bbuf = None
    if bound:
        bbuf = torch.zeros(cap * 6, dtype=torch.float32, device="cuda")
        g.bind_aabbs_device(bbuf.data_ptr(), cap)
    vs_b = np.float32(0.032)                     # build B: another (tiled, 32^3) grid, so that nothing of A is left in the buffers
    assert oracle.grid_info(v, vs_b)["dim"] == (32, 32, 32)
    for name, kw, status, keeps in failures:
        g.revoxelize(mesh, vs_b, materials=flags.get("materials", False))
        g.revoxelize(mesh, vs, **flags)          # build A (a list_async list stays unread until after the failure)
        kw = dict(kw)
        with pytest.raises(gpu.VxError) as ei:
            g.revoxelize(kw.pop("mesh", mesh), kw.pop("voxel_size"), **dict(flags, **kw))
        assert ei.value.status == status, name
        got = _read(gpu, g, rays, probes, cap)
        if keeps:
            _assert_same(exp, got, "%s after %s" % (flavour, name))
        else:
            _assert_empty(gpu, got, len(rays), len(probes))
        g.revoxelize(mesh, vs, **flags)          # A again: as on a fresh handle
        _assert_same(exp, _read(gpu, g, rays, probes, cap), "%s rebuilt after %s" % (flavour, name))
        if bound:
            torch.cuda.synchronize()
            assert bbuf.cpu().numpy()[: exp["aabbs_device"][0] * 6].tobytes() == exp["aabbs"]   # the build filled the caller's buffer


# ---------------------------------------------------------------------------------------------- spare words behind the mask
def _mask_words(g, n, mutable=False):
    """The first n words of the grid's device bitmask as an int32 torch tensor (the allocation holds num_words + 2)."""
    import torch

    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (g.bitmask_device_ptr(mutable=mutable), False), "version": 3, "strides": None}
    return torch.as_tensor(View(), device="cuda")


def _box_soup(x_cells, seed):
    """A dense soup in the box [0, x_cells] x [0, 20] x [0, 12] (pinned), for grids of x_cells / vs cells along x."""
    rng = np.random.default_rng(seed)
    n = 6000
    c = rng.uniform((0.0, 0.0, 0.0), (x_cells, 20.0, 12.0), (n, 3))
    tri = np.clip(c[:, None, :] + rng.uniform(-1.2, 1.2, (n, 3, 3)), 0.0, (x_cells, 20.0, 12.0))
    tri[0, 0] = (0.0, 0.0, 0.0)
    tri[1, 0] = (x_cells, 20.0, 12.0)
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def test_rebuild_smaller_grid_keeps_spare_words_zero(gpu):
    """big -> small -> big on one handle, with x a multiple of 32 (the tiled build mask) and not (the direct form): every build equals a
    fresh one, and the two words behind the mask (allocated nwords + 2) are zero."""
    import torch
    arrays = {"tiled": _box_soup(64.0, 3), "direct": _box_soup(63.0, 4)}    # x: 128 / 64 cells, 126 / 63 cells
    meshes = {k: gpu.Mesh.from_arrays(*a) for k, a in arrays.items()}
    seq = [("tiled", 0.5), ("tiled", 1.0), ("tiled", 0.5), ("direct", 1.0), ("tiled", 1.0), ("direct", 0.5), ("tiled", 1.0), ("direct", 1.0),
           ("tiled", 0.5)]
    for kind in (gpu.GRID_BOOL, gpu.GRID_VEC):
        g = None
        prev = None
        stale = 0
        for name, vs in seq:
            vs = np.float32(vs)
            v, t = arrays[name]
            mesh = meshes[name]
            if g is None:
                g = gpu.Grid.voxelize(mesh, vs, kind)
            else:
                g.revoxelize(mesh, vs)
            fresh = gpu.Grid.voxelize(mesh, vs, kind)
            w = g.bitmask()
            ow = oracle.build_bool(v, t, vs)[0]
            assert np.array_equal(w, ow) and np.array_equal(fresh.bitmask(), ow)
            assert g.aabbs().tobytes() == fresh.aabbs().tobytes()
            nw = len(w)
            if prev is not None and len(prev) >= nw + 2:
                stale += bool(prev[nw:nw + 2].any())     # the previous build left bits where this one's spare words are
            torch.cuda.synchronize()
            tail = _mask_words(g, nw + 2).cpu().numpy().view(np.uint32)
            assert np.array_equal(tail[:nw], ow) and not tail[nw:].any(), (kind, name, float(vs), tail[nw:])
            prev = w
        assert stale >= 2


def _floor_and_ceiling(x_cells, n=300, seed=8):
    """Small triangles near z = 0 and z = 64 only, in the box [0, x_cells] x [0, 64] x [0, 64] (pinned): word shards by rank of 4 whose z
    slab lies in between hold no triangle at all."""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform((0.0, 0.0, 0.3), (x_cells, 64.0, 1.4), (n, 3)), rng.uniform((0.0, 0.0, 62.6), (x_cells, 64.0, 63.7), (n, 3))])
    tri = np.clip(c[:, None, :] + rng.uniform(-1.1, 1.1, (2 * n, 3, 3)) * (1.0, 1.0, 0.25), 0.0, (x_cells, 64.0, 64.0))
    tri[0, 0] = (0.0, 0.0, 0.0)
    tri[n, 0] = (x_cells, 64.0, 64.0)
    v = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32))
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("x_cells", [64.0, 63.0], ids=["tiled", "direct"])
def test_word_shard_without_triangles(gpu, x_cells):
    """Word shards by rank whose z slab holds no triangle (no work unit at all), on the tiled shard path (x % 32 == 0) and the direct one:
    the mask is the oracle's words of the shard and zeros elsewhere -- on a handle whose previous build filled the mask, and on fresh
    handles whose blocks come back from the pool with another grid's bits -- and the two spare words behind it are zero."""
    import torch
    v, t = _floor_and_ceiling(x_cells)
    vs = np.float32(1.0)
    mesh = gpu.Mesh.from_arrays(v, t)
    ow = oracle.build_bool(v, t, vs)[0]
    nw = len(ow)
    world = 4
    empty_ranks = 0

    def check(g, rank):
        wb, we, _ = gpu.shard_words(nw, rank, world)
        exp = np.zeros_like(ow)
        exp[wb:we] = ow[wb:we]
        w = g.bitmask()
        torch.cuda.synchronize()
        tail = _mask_words(g, nw + 2).cpu().numpy().view(np.uint32)
        assert np.array_equal(w, exp) and np.array_equal(tail[:nw], exp) and not tail[nw:].any(), (x_cells, rank, int((w != exp).sum()), tail[nw:])
        return not ow[wb:we].any()

    # one handle: a full build, then every rank's shard
    g = gpu.Grid.voxelize(mesh, vs)
    for rank in range(world):
        g.revoxelize(mesh, vs)
        assert np.array_equal(g.bitmask(), ow)
        g.revoxelize(mesh, vs, shard=(rank, world))
        empty_ranks += check(g, rank)
    # fresh handles, each after a full grid of the same size was freed
    for rank in range(world):
        full = gpu.Grid.voxelize(mesh, vs)
        _mask_words(full, nw + 2, mutable=True).fill_(-1)
        torch.cuda.synchronize()
        full.free()
        empty_ranks += check(gpu.Grid.voxelize(mesh, vs, shard=(rank, world)), rank)
    assert empty_ranks == 4   # ranks 1 and 2, on both kinds of handle


# ---------------------------------------------------------------------------------------------- 2^32 edges
# Every total of a count at or above 2^32 - 1 is refused (VX_ERR_CAPACITY): the prefix scans that produce them carry 64-bit totals
# (tests/test_gpu_scan.py); here the guards behind them through the public API.
UNITS_MSG = "more than 2^32 candidate row segments: shard the mesh or the grid"
OCC_MSG = "more than 2^32 occupied voxels"
F = np.float32


def _cand_axis(a, b, c, gmin, vsize, dim):
    """cand_axis (vx_math.h; VoxelBuilder.hpp:175-184) in float32"""
    tmn, tmx = min(a, b, c), max(a, b, c)
    s0 = int(F(F(tmn - gmin) / vsize))
    e0 = int(F(F(tmx - gmin) / vsize)) + 2
    return max(s0, 0), min(e0, int(dim))


def _trim_axis(a0, a1, a2, org, vs, half, s, e):
    """trim_axis (vx_kernels.hip): drop end slabs that the box-axis test separates"""
    def sep(i):
        c = F(org + F(F(F(i) + F(0.5)) * vs))
        p = (F(a0 - c), F(a1 - c), F(a2 - c))
        return min(p) > half or max(p) < -half
    while e > s and sep(e - 1):
        e -= 1
    while e > s and sep(s):
        s += 1
    return s, e


def units_per_triangle(tri, gi, vs, sat=0):
    """k_tri_setup's unit count of one triangle (float32 vertices [3, 3]): rows of the trimmed candidate box cut at multiples of 32 in x"""
    vs = F(vs)
    half = F(vs * F(0.5))
    vsize = F(half * F(2.0)) if sat == 0 else vs
    org = [F(x) for x in gi["bmin"]]
    rng = []
    for a in range(3):
        v = [F(tri[k][a]) for k in range(3)]
        s, e = _cand_axis(*v, org[a], vsize, gi["dim"][a])
        rng.append(_trim_axis(*v, org[a], vs, half, s, e))
    (xs, xe), (ys, ye), (zs, ze) = rng
    nx, ny, nz = max(xe - xs, 0), max(ye - ys, 0), max(ze - zs, 0)
    if not (nx and ny and nz):
        return 0
    nseg = ((xs + nx - 1) >> 5) - (xs >> 5) + 1
    return min(nseg * ny * nz, 0xFFFFFFFF)


def _units_mesh():
    """4096 copies of a triangle of 2^20 units over a 4096 x 4096 x 2 grid (2^32 units, all in one 16384-triangle scan tile), then one
    small triangle: the true total is 2^32 + a few units, and a 32-bit tile sum reads it as those few"""
    big = np.array([[0.0, 0.0, 0.0], [4096.0, 0.0, 1.0], [0.0, 4096.0, 2.0]], np.float32)
    small = np.array([[100.25, 200.25, 0.25], [101.75, 200.5, 0.5], [100.5, 201.75, 0.75]], np.float32)
    tri = np.concatenate([np.repeat(big[None], 4096, 0), small[None]])
    v = np.ascontiguousarray(tri.reshape(-1, 3))
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), np.float32(1.0), big, small


def test_units_total_past_2_32(gpu):
    """a unit total just past 2^32 in one scan tile: VX_ERR_CAPACITY from the grid build, a triangle shard and the Octree (a wrapped total
    used to return VX_OK with the mask of a few units)"""
    v, t, vs, big, small = _units_mesh()
    gi = oracle.grid_info(v, vs)
    assert gi["dim"] == (4096, 4096, 2)
    ub, us = units_per_triangle(big, gi, vs), units_per_triangle(small, gi, vs)
    assert ub == 1 << 20 and 0 < us < 64
    assert 4096 * ub + us == (1 << 32) + us
    mesh = gpu.Mesh.from_arrays(v, t)
    for what, build in (("grid", lambda: gpu.Grid.voxelize(mesh, vs)), ("vec", lambda: gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)),
                        ("triangle shard", lambda: gpu.Grid.voxelize(mesh, vs, tris=(0, len(t)))),
                        ("octree", lambda: gpu.Octree(mesh, vs))):
        with pytest.raises(gpu.VxError) as ei:
            build()
        assert ei.value.status == ERR_CAPACITY and ei.value.message == UNITS_MSG, what


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_units_total_past_2_32_rebuild(gpu, flavour):
    """revoxelize into a live handle of every flavour with the unit total past 2^32: VX_ERR_CAPACITY, the empty grid of the failure
    contract, and the next build equals a fresh handle's"""
    import torch
    kind_name, flags, bound = FLAVOURS[flavour]
    kind = getattr(gpu, kind_name)
    v, t, vs = _scene_a()
    mesh = gpu.Mesh.from_arrays(v, t)
    cv, ct, cvs, _, _ = _units_mesh()
    cmesh = gpu.Mesh.from_arrays(cv, ct)
    if flags.get("materials"):
        mesh.set_materials(*_materials(len(t))[:2])
        cmesh.set_materials(*_materials(len(ct))[:2])
    gi = oracle.grid_info(v, vs)
    rays = vx_scenes.random_rays(3000, gi["bmin"], gi["bmin"] + np.array(gi["dim"], np.float32) * vs, seed=31)
    probes = [tuple(int(x) for x in np.random.default_rng(k).integers(0, gi["dim"])) for k in range(12)]
    ref = gpu.Grid.voxelize(mesh, vs, kind, materials=flags.get("materials", False))
    cap = ref.describe()["set_calls"] + 64
    exp = _read(gpu, ref, rays, probes, cap)
    ref.free()
    g = gpu.Grid.voxelize(mesh, vs, kind, materials=flags.get("materials", False))
    bbuf = None
    if bound:
        bbuf = torch.zeros(cap * 6, dtype=torch.float32, device="cuda")
        g.bind_aabbs_device(bbuf.data_ptr(), cap)
    g.revoxelize(mesh, vs, **flags)
    with pytest.raises(gpu.VxError) as ei:
        g.revoxelize(cmesh, cvs, **flags)
    assert ei.value.status == ERR_CAPACITY and ei.value.message == UNITS_MSG
    _assert_empty(gpu, _read(gpu, g, rays, probes, cap), len(rays), len(probes))
    with pytest.raises(gpu.VxError) as ei:
        g.revoxelize(cmesh, cvs, tris=(0, len(ct)), **flags)
    assert ei.value.status == ERR_CAPACITY
    g.revoxelize(mesh, vs, **flags)
    _assert_same(exp, _read(gpu, g, rays, probes, cap), "%s rebuilt after the unit total" % flavour)
    g.free()


def _down_rays(cells, X, Y):
    """rays from above (z = 3) down through the centres of cells (x, y, 0), slightly oblique"""
    i = np.asarray(cells, np.uint64)
    x = (i % np.uint64(X)).astype(np.float32) + np.float32(0.5)
    y = (i // np.uint64(X) % np.uint64(Y)).astype(np.float32) + np.float32(0.5)
    n = len(i)
    return np.ascontiguousarray(np.stack([x, y, np.full(n, 3.0, np.float32), np.full(n, 1e-6, np.float32), np.full(n, -1e-6, np.float32),
                                          np.full(n, -1.0, np.float32)], 1))


def _cell_aabbs(cells, X, Y):
    i = np.asarray(cells, np.uint64)
    mn = np.stack([(i % np.uint64(X)), (i // np.uint64(X) % np.uint64(Y)), np.zeros_like(i)], 1).astype(np.float32)
    a = np.zeros(len(i), dtype=oracle.AABB)
    a["mn"], a["mx"] = mn, mn + np.float32(1.0)
    return a


def _full_grid_less(gpu, X, Y, cleared):
    """a Bool grid X x Y x 1 (vs 1, origin 0) with every cell set but `cleared`, written through the mutable device pointer after a fill
    of the whole word array (padding bits included) and refreshed"""
    import torch
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, 1, 1.0)
    nw = g.describe()["num_words"]
    m = _mask_words(g, nw, mutable=True)
    m.fill_(-1)
    for c in cleared:
        w = int(m[c // 32].item()) & 0xFFFFFFFF
        m[c // 32] = int(np.uint32(w & ~(1 << (c % 32))).view(np.int32))
    torch.cuda.synchronize()
    del m
    return g, nw


@pytest.mark.parametrize("X,Y", [(65535, 65537), (65535, 65535)], ids=["wp16", "word_prefix"])
def test_occupied_and_rays_near_2_32(gpu, X, Y):
    """2^32 - 1 cells (64-bit ray indices; a word count divisible by 16: k_rank's wp16 path) and 65535^2 cells (the plain word_prefix
    path): every cell set but one gives occupied = N - 1, exact; rays at cells near the end and around rank 2^31 return primitive ids
    bit-equal to oracle.voxel_rank, t bit-equal to the slab formula of the hit cell, the cube normal and the shadow flag; the cleared cell
    is a miss."""
    N = X * Y
    c0 = N - 5
    g, nw = _full_grid_less(gpu, X, Y, [c0])
    assert (nw % 16 == 0) == (X * Y == (1 << 32) - 1)
    g.refresh()
    assert g.describe()["occupied"] == N - 1
    if N == (1 << 32) - 1:
        assert N - 1 == 0xFFFFFFFE
    cells = [N - 1, N - 2, N - 3, N - 4, c0, c0 - 1, c0 - 17, N - 32 * 16 - 1, 1 << 31, (1 << 31) + 1, (1 << 31) - 1, (1 << 31) + 12345, 3 << 30, 0, 31, 32]
    rays = _down_rays(cells, X, Y)
    ex = g.trace_ex(rays, want=("t", "prim", "normal"))
    words = g.bitmask()
    last = (0xFFFFFFFF if N % 32 == 0 else (1 << (N % 32)) - 1) & ~((1 << (c0 % 32)) if c0 // 32 == nw - 1 else 0)
    assert int(words[-1]) == last   # the padding bits were cleared by refresh
    want_prim = oracle.voxel_rank(words, np.array([c if c != c0 else 0xFFFFFFFFFFFFFFFF for c in cells], np.uint64))
    del words
    hit = np.array([c != c0 for c in cells])
    assert np.array_equal(ex["prim"][hit], want_prim[hit])
    assert (ex["t"][~hit] <= 0).all()
    assert want_prim[hit].max() == N - 2 and (want_prim[hit] >= (1 << 31)).sum() >= 8
    aabbs = _cell_aabbs(cells, X, Y)
    for k in np.flatnonzero(hit):    # t and normal of the one cell the ray enters
        bt, bp = oracle.trace_brute(aabbs[k:k + 1], rays[k:k + 1])
        assert ex["t"][k].tobytes() == bt.tobytes() and bp[0] == 0, k
        assert np.array_equal(ex["normal"][k:k + 1], oracle.cube_normals(aabbs[k:k + 1], bp, rays[k:k + 1], bt)), k
    t2, p2, _ = g.trace(rays)
    assert np.array_equal(t2, ex["t"]) and np.array_equal(p2[hit], ex["prim"][hit])
    sh = g.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"]
    assert np.array_equal(sh.astype(bool), hit)
    g.free()


def test_occupied_at_2_32(gpu):
    """2^32 - 1 cells all set: VX_ERR_CAPACITY "more than 2^32 occupied voxels"; 65535 x 65536 cells (4294901760) all set: accepted and
    exact"""
    g, _ = _full_grid_less(gpu, 65535, 65537, [])
    with pytest.raises(gpu.VxError) as ei:
        g.refresh()
    assert ei.value.status == ERR_CAPACITY and ei.value.message == OCC_MSG
    g.free()
    g, nw = _full_grid_less(gpu, 65535, 65536, [])
    g.refresh()
    assert g.describe()["occupied"] == 65535 * 65536 == 4294901760
    g.free()


def test_render_pixels_at_2_32(gpu):
    """vx_render_frame* with width * height >= 2^32 - 1: VX_ERR_CAPACITY before anything is allocated or queued"""
    import ctypes as C
    v, t = vx_scenes.rotated_cube()
    grid = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), np.float32(0.09))
    r = gpu.Renderer(grid)
    eye = np.eye(4, dtype=np.float32)
    dummy = np.zeros(16, np.uint32)
    for w, h in ((65536, 65536), (65535, 65537), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF)):
        a, keep = r._args((eye, eye, w, h), None)
        a.rgba = dummy.ctypes.data
        for fn in (gpu.lib().vx_render_frame, gpu.lib().vx_render_frame_device):
            before = gpu.device_allocations()
            st = fn(r.h, C.byref(a))
            assert st == ERR_CAPACITY and gpu.lib().vx_last_error().decode() == "more than 2^32 pixels", (w, h)
            assert gpu.device_allocations() == before
    assert not dummy.any()
    r.free()


@pytest.mark.parametrize("X", [33, 63, 64, 1])
def test_mask_padding_bits(gpu, X):
    """bits past X*Y*Z in the last word of an externally written mask are not cells: refresh clears them (voxhip.h,
    vx_grid_bitmask_device_mut), so occupied, the AABB list and the rays see exactly the grid's cells"""
    import torch
    g = gpu.Grid.create(gpu.GRID_BOOL, X, 1, 1, 1.0)
    nw = g.describe()["num_words"]
    assert nw == (X + 31) // 32
    m = _mask_words(g, nw, mutable=True)
    m.fill_(-1)
    torch.cuda.synchronize()
    del m
    g.refresh()
    d = g.describe()
    assert d["occupied"] == X
    w = g.bitmask()
    want = np.full(nw, 0xFFFFFFFF, np.uint32)
    if X % 32:
        want[-1] = (1 << (X % 32)) - 1
    assert np.array_equal(w, want)
    a = g.aabbs()
    assert len(a) == X and a["mx"][:, 0].max() == np.float32(X)
    rays = np.array([[X + 40.0, 0.5, 0.5, -1.0, 1e-7, -1e-7]], np.float32)   # along -x from beyond the grid: the first hit is cell X - 1
    tt, pp, _ = g.trace(rays)
    assert pp[0] == X - 1 and tt[0] > 0
    g.free()
