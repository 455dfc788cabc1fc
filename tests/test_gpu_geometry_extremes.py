"""GPU tests of the builders on geometry at its extremes (include/voxhip.h, "geometry at its extremes"), over the
families of tests/geometry_extremes.py:
  - a mesh with a NaN or infinite vertex is REFUSED by every voxelizing entry point (any vertex) and by the BVH build (a referenced
    vertex): VX_ERR_INVALID_ARG, "non-finite", the handle left empty, nothing leaked;
  - a finite outlier (2^100, +-FLT_MAX/2, +-0.75 FLT_MAX) is ordinary input: BVH and TLAS stay bit-equal to the brute forces over all
    triangles, the voxelizer and the octree report the size of the grid as they always did;
  - the voxelizer is bit-identical to the oracle on scene * 2^k down through gradual underflow, and every ray query scales with it.
Every case is small: at most 2317 + 8 triangles, 3000 rays, 37 cells per axis."""
import numpy as np
import pytest

import geometry_extremes as gx
import instance_ref
import mesh_multihit_ref as mmr
import mesh_ref
import multihit_ref as mr
import oracle
import ray_extremes as rx
from test_gpu_limits import ERR_CAPACITY, ERR_INVALID_ARG, ERR_MORTON_BITS, _assert_empty, _assert_same, _read
from test_gpu_mesh_trace import check_closest, check_structure

pytestmark = pytest.mark.gpu

F = np.float32
K = 4
POISONS = [(k, v) for k in gx.POISON_KINDS for v in gx.POISON_BITS]
POISON_IDS = ["%s_%s" % p for p in POISONS]
LEAVES = (1, 0)


def refused(vx, fn, what):
    with pytest.raises(vx.VxError) as e:
        fn()
    assert e.value.status == ERR_INVALID_ARG and "non-finite" in e.value.message, "%s: status %d, %r" % (what, e.value.status, e.value.message)


def device_mesh(vx, v, t):
    import torch
    dv, dt = torch.from_numpy(np.array(v)).cuda(), torch.from_numpy(np.array(t)).cuda()
    torch.cuda.synchronize()
    return vx.Mesh.from_device(dv.data_ptr(), len(v), dt.data_ptr(), len(t), keep=(dv, dt))


def multi_voxelize(vx, mesh, vs):
    mc = vx.Multi(mesh, [0, 0])
    try:
        return mc.voxelize(vs)
    finally:
        mc.free()


def voxelizers(vx, mesh, vs, host=True):
    """every voxelizing entry point on the mesh, as (name, callable)"""
    kinds = (("bool", vx.GRID_BOOL), ("aabbstruct", vx.GRID_AABBSTRUCT), ("vec", vx.GRID_VEC))
    out = [("voxelize %s sat %d" % (n, sat), lambda k=k, sat=sat: vx.Grid.voxelize(mesh, vs, k, sat_variant=sat)) for n, k in kinds for sat in (0, 1)]
    out.append(("octree", lambda: vx.Octree(mesh, vs)))
    if host:                                                    # the multi-device entries upload a host mesh themselves
        out.append(("voxelize_multi", lambda: vx.Grid.voxelize_multi(mesh, vs, [0, 0, 0])))
        out.append(("multi_voxelize", lambda: multi_voxelize(vx, mesh, vs)))
    return out


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,value", POISONS, ids=POISON_IDS)
def test_poisoned_mesh_is_refused_by_every_builder(gpu, kind, value):
    live = gpu.device_live_blocks()
    for name in gx.SCENES:
        m = gx.poisoned(name, kind, value)
        vs = gx.VOXEL_SIZE[name]
        cv, ct = gx.scene(name)
        clean = gpu.Mesh.from_arrays(cv, ct)
        for host in (True, False):
            mesh = gpu.Mesh.from_arrays(m.v, m.t) if host else device_mesh(gpu, m.v, m.t)
            what = "%s %s %s %s" % (name, kind, value, "host" if host else "borrowed")
            for n, fn in voxelizers(gpu, mesh, vs, host):
                refused(gpu, fn, what + " " + n)
            refused(gpu, lambda: mesh.bvh(), what + " bvh")
            refused(gpu, lambda: mesh.bvh(max_leaf=1), what + " bvh max_leaf 1")
            b = clean.bvh()
            refused(gpu, lambda: b.build_into(mesh), what + " build_into")
            rays = gx.mesh_rays(name)[:256]
            assert b.num_triangles == 0 and b.num_nodes == 0 and np.all(b.trace(rays)[0] == -1.0), what   # a failed rebuild leaves the empty BVH
            b.build_into(clean)
            fresh = clean.bvh()
            assert np.array_equal(b.nodes(), fresh.nodes()) and np.array_equal(b.trace(rays)[0], fresh.trace(rays)[0]), what
            b.free()
            fresh.free()
            mesh.free()
        clean.free()
    assert gpu.device_live_blocks() == live


@pytest.mark.parametrize("kind,value", POISONS, ids=POISON_IDS)
def test_refused_rebuild_leaves_the_empty_grid(gpu, kind, value):
    """vx_voxelize_into on a handle that holds another build: the failure is of the header's second class -- the handle is empty through
    every reader, every ray misses, and the next build of the clean mesh equals a fresh one byte for byte"""
    i = POISONS.index((kind, value))
    name = gx.GRID_SCENES[i % 2]
    gk = (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC)[i % 3]
    sat = (i // 2) % 2
    vs = gx.VOXEL_SIZE[name]
    cv, ct = gx.scene(name)
    clean = gpu.Mesh.from_arrays(cv, ct)
    sc = rx.grid_scene(name)
    rays = gx.grid_rays(name)
    rng = np.random.default_rng(i)
    probes = [tuple(int(rng.integers(0, n)) for n in sc.gi["dim"]) for _ in range(8)]
    ref = gpu.Grid.voxelize(clean, vs, gk, sat_variant=sat)
    cap = ref.describe()["set_calls"] + 64
    exp = _read(gpu, ref, rays, probes, cap)
    g = gpu.Grid.voxelize(clean, F(vs * 2), gk, sat_variant=sat)                 # another build in the handle
    for referenced in (True, False):
        m = gx.poisoned(name, kind, value, referenced)
        for host in (True, False):
            bad = gpu.Mesh.from_arrays(m.v, m.t) if host else device_mesh(gpu, m.v, m.t)
            refused(gpu, lambda: g.revoxelize(bad, vs, sat_variant=sat), "%s %s %s revoxelize" % (name, kind, value))
            _assert_empty(gpu, _read(gpu, g, rays, probes, cap), len(rays), len(probes))
            assert not g.trace_multi(rays, max_hits=K, want=("count",))["count"].any()
            g.revoxelize(clean, vs, sat_variant=sat)
            _assert_same(exp, _read(gpu, g, rays, probes, cap), "rebuilt after %s %s" % (kind, value))
            bad.free()


_clean_bvh = {}


def clean_bvh(vx, name, leaf):
    """(Bvh, nodes, leaf order, closest / any / multi on mesh_rays) of the clean scene, one per module"""
    key = (name, leaf)
    if key not in _clean_bvh:
        v, t = gx.scene(name)
        b = vx.Mesh.from_arrays(v, t).bvh(max_leaf=leaf)
        rays = gx.mesh_rays(name)
        _clean_bvh[key] = (b, b.nodes(), b.leaf_triangles(), b.trace_ex(rays, want=("t", "prim", "bary")),
                           b.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"], b.trace_multi(rays, max_hits=K, want=("t", "prim", "bary", "count")))
    return _clean_bvh[key]


@pytest.mark.parametrize("kind,value", POISONS, ids=POISON_IDS)
def test_unreferenced_poison(gpu, kind, value):
    """poisoned vertices that no triangle uses: the voxelizer and the octree take the box over ALL vertices and refuse; the BVH never
    reads them -- its nodes, leaf order and traces are those of the clean mesh"""
    for name in gx.SCENES:
        m = gx.poisoned(name, kind, value, referenced=False)
        assert np.array_equal(m.t, m.clean_t)
        vs = gx.VOXEL_SIZE[name]
        rays = gx.mesh_rays(name)
        for host in (True, False):
            mesh = gpu.Mesh.from_arrays(m.v, m.t) if host else device_mesh(gpu, m.v, m.t)
            for n, fn in voxelizers(gpu, mesh, vs, host):
                refused(gpu, fn, "%s unreferenced %s %s %s" % (name, kind, value, n))
            for leaf in LEAVES:
                cb, nodes, order, cl, sh, mu = clean_bvh(gpu, name, leaf)
                b = mesh.bvh(max_leaf=leaf)
                assert np.array_equal(b.nodes(), nodes) and np.array_equal(b.leaf_triangles(), order)
                got = b.trace_ex(rays, want=("t", "prim", "bary"))
                assert rx.first_difference(got, cl, rays) is None
                assert np.array_equal(b.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"], sh)
                assert rx.first_difference(b.trace_multi(rays, max_hits=K, want=("t", "prim", "bary", "count")), mu, rays) is None
                b.free()
            mesh.free()


def test_clean_bvh_equals_the_brute_force(gpu):
    """what test_unreferenced_poison compares with is itself the reference's answer"""
    for name in gx.SCENES:
        v, t = gx.scene(name)
        rays = gx.mesh_rays(name)
        for leaf in LEAVES:
            check_closest(clean_bvh(gpu, name, leaf)[0], v, t, rays, "%s clean max_leaf %d" % (name, leaf))


# ---- outliers -----------------------------------------------------------------------------------------------------------------------------
_outlier_ref = {}


def outlier_ref(name, mag, referenced):
    key = (name, mag, referenced)
    if key not in _outlier_ref:
        m = gx.outlier(name, mag, referenced)
        rays = gx.mesh_rays(name)
        hits = mmr.all_hits(m.v, m.t, rays)
        multi = mmr.select(hits, K)
        multi.pop("instance")
        _outlier_ref[key] = (mesh_ref.closest(m.v, m.t, rays), mesh_ref.any_hit(m.v, m.t, rays), multi, hits)
    return _outlier_ref[key]


@pytest.mark.parametrize("referenced", [True, False], ids=["referenced", "unreferenced"])
@pytest.mark.parametrize("mag", gx.OUTLIERS)
@pytest.mark.parametrize("name", gx.BVH_SCENES)
def test_outlier_bvh(gpu, name, mag, referenced):
    m = gx.outlier(name, mag, referenced)
    rays = gx.mesh_rays(name)
    closest, anyhit, multi, hits = outlier_ref(name, mag, referenced)
    if referenced:
        assert m.stray[hits.prim].any()                              # the reference does accept triangles that reach to the outlier
    mesh = gpu.Mesh.from_arrays(m.v, m.t)
    for leaf in LEAVES:
        what = "%s outlier %s max_leaf %d" % (name, mag, leaf)
        b = mesh.bvh(max_leaf=leaf)
        check_structure(b, m.v, m.t)
        check_closest(b, m.v, m.t, rays, what, closest)
        assert np.array_equal(b.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"], anyhit), what + " any_hit"
        gm = b.trace_multi(rays, max_hits=K, want=("t", "prim", "bary", "count"))
        diff = rx.first_difference(gm, multi, rays)
        assert diff is None, what + " multi: " + diff
        b.free()
    # the voxelizer and the octree on the same mesh: the grid is too large, as for any mesh of that extent
    vs = gx.VOXEL_SIZE[name]
    for gk in (gpu.GRID_BOOL, gpu.GRID_VEC):
        for sat in (0, 1):
            with pytest.raises(gpu.VxError) as e:
                gpu.Grid.voxelize(mesh, vs, gk, sat_variant=sat)
            assert e.value.status == ERR_CAPACITY, (e.value.status, e.value.message)
    with pytest.raises(gpu.VxError) as e:
        gpu.Octree(mesh, vs)
    assert e.value.status == ERR_MORTON_BITS and e.value.message == "We support up to 21 bits per axis (max 2^21 voxels per dimension)!"
    mesh.free()


@pytest.mark.parametrize("mag", gx.OUTLIERS)
@pytest.mark.parametrize("name", gx.BVH_SCENES)
def test_outlier_tlas(gpu, name, mag):
    sc = gx.outlier_tlas(name, mag)
    rays = gx.tlas_rays(name)
    rt, ri, rp, rb = instance_ref.closest(sc.meshes, sc.inst, rays)
    hits = mmr.all_hits_tlas(sc.meshes, sc.inst, rays)
    on_outlier = sc.inst["blas"][hits.inst] == 0
    assert sc.stray[hits.prim[on_outlier]].any() and (~on_outlier).any()
    for leaf in LEAVES:
        what = "%s outlier %s tlas max_leaf %d" % (name, mag, leaf)
        blas = [gpu.Bvh(gpu.Mesh.from_arrays(v, t), max_leaf=leaf) for v, t in sc.meshes]
        tl = gpu.Tlas(blas, sc.inst)
        got = tl.trace_ex(rays, want=("t", "instance", "prim", "bary"))
        diff = rx.first_difference(got, {"t": rt, "instance": ri, "prim": rp, "bary": rb}, rays)
        assert diff is None, what + " closest: " + diff
        sh = tl.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(sh, instance_ref.any_hit(sc.meshes, sc.inst, rays)), what + " any_hit"
        gm = tl.trace_multi(rays, max_hits=K, want=("t", "instance", "prim", "bary", "count"))
        diff = rx.first_difference(gm, mmr.select(hits, K), rays)
        assert diff is None, what + " multi: " + diff
        tl.free()
        for b in blas:
            b.free()


# ---- scale --------------------------------------------------------------------------------------------------------------------------------
SCALES = [(sat, k) for sat in (1, 0) for k in gx.SCALE_K[sat]]


@pytest.mark.parametrize("sat,k", SCALES, ids=["sat%d_k%+d" % s for s in SCALES])
@pytest.mark.parametrize("name", gx.GRID_SCENES)
def test_voxelizer_scaled(gpu, name, sat, k):
    s = gx.scaled(name, k)
    ow, calls, gi = oracle.build_bool(s.v, s.t, s.vs, threads=0, sat=sat)
    oa = oracle.bool_aabbs(ow, gi, s.vs)
    assert (calls, len(oa)) == gx.ORACLE_TABLE[name, sat][k]
    mesh = gpu.Mesh.from_arrays(s.v, s.t)
    g = gpu.Grid.voxelize(mesh, s.vs, gpu.GRID_BOOL, sat_variant=sat)
    d = g.describe()
    print("%s sat %d k %+d: gpu set_calls %d occupied %d, oracle %d %d" % (name, sat, k, d["set_calls"], d["occupied"], calls, len(oa)))
    assert d["dim"] == gi["dim"] and np.array_equal(g.bitmask(), ow), "bitmask"
    assert d["set_calls"] == calls and d["occupied"] == len(oa)
    ga = g.aabbs()
    assert ga.tobytes() == oa.tobytes(), "Bool list"
    gv = gpu.Grid.voxelize(mesh, s.vs, gpu.GRID_VEC, sat_variant=sat)
    assert gv.aabbs().tobytes() == oracle.build_vec(s.v, s.t, s.vs, threads=0, sat=sat).tobytes(), "Vec list"
    o = gpu.Octree(mesh, s.vs)                                  # (the Octree has one SAT of its own: the same build at either sat)
    assert np.array_equal(o.items(), oracle.octree(s.v, s.t, s.vs, threads=4)["items"]), "octree items"
    o.free()
    if k in gx.TRACE_K:
        rays = gx.scaled_rays(gx.grid_rays(name), k)
        tmin, tmax = gx.scaled_interval(k)
        tt, pp, nh = g.trace(rays, tmin=tmin, tmax=tmax)
        ot, op = oracle.trace_brute(ga, rays, tmin, tmax)
        assert (ot > 0).mean() > 0.2
        diff = rx.first_difference({"t": tt, "prim": pp}, {"t": ot, "prim": op}, rays)
        assert diff is None and nh == int((ot > 0).sum()), diff
        mrays = rays[:: 4]
        times = np.concatenate([mr.hit_times(ga, mrays[i:i + 32], chunk=32) for i in range(0, len(mrays), 32)])
        et, ep, ec = mr.select(times, K, tmin=tmin, tmax=tmax)
        gm = g.trace_multi(mrays, max_hits=K, tmin=tmin, tmax=tmax, want=("t", "prim", "count"))
        diff = rx.first_difference(gm, {"t": et, "prim": ep, "count": ec}, mrays)
        assert diff is None, diff
    for h in (g, gv, mesh):
        h.free()


@pytest.mark.parametrize("k", [-30, 30])
@pytest.mark.parametrize("name", gx.BVH_SCENES)
def test_bvh_scaled(gpu, name, k):
    """scene * 2^k, ray origins * 2^k, interval * 2^k: bit-equal to the brute force on that same scaled input"""
    v, t = gx.scene(name)
    sv = np.ldexp(v, k).astype(F)
    rays = gx.scaled_rays(gx.mesh_rays(name), k)
    tmin, tmax = gx.scaled_interval(k)
    rt, rp, rb = mesh_ref.closest(sv, t, rays, tmin, tmax)
    assert (rt > 0).mean() > 0.1
    mesh = gpu.Mesh.from_arrays(sv, t)
    for leaf in LEAVES:
        b = mesh.bvh(max_leaf=leaf)
        got = b.trace_ex(rays, tmin=tmin, tmax=tmax, want=("t", "prim", "bary"))
        diff = rx.first_difference(got, {"t": rt, "prim": rp, "bary": rb}, rays)
        assert diff is None, "%s k %+d max_leaf %d: %s" % (name, k, leaf, diff)
        sh = b.trace_ex(rays, tmin=tmin, tmax=tmax, any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(sh, mesh_ref.any_hit(sv, t, rays, tmin, tmax))
        b.free()
    mesh.free()
