"""GPU tests of the triangle ray queries (vx_bvh_*, k_bvh_trace): first hit, barycentrics, normals, shadow queries, camera rays and the
compacted hit list on the device-built BVH, against the numpy brute force of tests/mesh_ref.py -- t, prim and bary bit-equal."""
import os
import subprocess

import numpy as np
import pytest

import mesh_ref
import oracle
import vx_scenes
from test_gpu_octree_trace import zero_component_rays
from test_gpu_parity import axis_rays, inside_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
LEAF_SIZES = [1, 4, 16, 0]            # 0 = the library default
INVALID_ARG, UNSUPPORTED = 1, 9


def floor_scene():
    """The cube standing on a floor of two axis-aligned triangles at y = -1 (zero-thickness boxes)."""
    cv, ct = vx_scenes.cube()
    fv = np.float32([[-4, -1, -4], [4, -1, -4], [4, -1, 4], [-4, -1, 4]])
    ft = np.int32([[0, 1, 2], [0, 2, 3]])
    return np.concatenate([cv, fv]).astype(np.float32), np.concatenate([ct, ft + len(cv)]).astype(np.int32)


def scene(name):
    if name == "floor":
        return floor_scene()
    return vx_scenes.scene(name)


def mesh_gi(v, n_cells=32):
    bmin, bmax = v.min(0).astype(np.float32), v.max(0).astype(np.float32)
    vs = float(max((bmax - bmin).max(), 1e-3)) / n_cells
    return {"dim": tuple(int(x) for x in np.maximum(np.ceil((bmax - bmin) / vs), 1)), "bmin": bmin, "bmax": bmax}, vs


def vertex_rays(v, t, n, seed):
    """Rays aimed exactly at mesh vertices and at edge midpoints (through shared vertices / edges)."""
    rng = np.random.default_rng(seed)
    bmin, bmax = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ctr, R = (bmin + bmax) / 2, 2.5 * max(np.linalg.norm(bmax - bmin), 1e-3)
    tri = t[rng.integers(0, len(t), n)]
    k = rng.integers(0, 3, n)
    a = v[tri[np.arange(n), k]].astype(np.float64)
    b = v[tri[np.arange(n), (k + 1) % 3]].astype(np.float64)
    tgt = np.where((np.arange(n) % 2 == 0)[:, None], a, (a + b) / 2)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (ctr + R * d).astype(np.float32)
    dr = tgt - o.astype(np.float64)
    dr = (dr / np.linalg.norm(dr, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([o, dr], axis=1))


def grazing_floor_rays(n, seed, y=-1.0):
    """Rays (nearly) in the floor plane y = -1: exactly in it, just above / below it, descending at tiny slopes."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-6, 6, n), np.full(n, y), rng.uniform(-6, 6, n)], 1)
    o[:, 1] += rng.choice([0.0, 1e-6, -1e-6, 1e-3, 1e-2], n)
    d = np.stack([rng.uniform(-1, 1, n), np.zeros(n), rng.uniform(-1, 1, n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 1] = rng.choice([0.0, -0.0, -1e-7, -1e-4, -1e-2, 1e-5], n)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32))


def ray_families(v, t, n, seed):
    gi, vs = mesh_gi(v)
    return {"random": vx_scenes.random_rays(n, gi["bmin"], gi["bmax"], seed=seed), "vertex": vertex_rays(v, t, n, seed + 1),
            "axis": axis_rays(gi, vs, n // 2, seed + 2), "zero": zero_component_rays(gi, vs, n // 2, seed + 3),
            "inside": inside_rays(gi, vs, n, seed + 4), "grazing": grazing_floor_rays(n // 2, seed + 5, float(gi["bmin"][1]))}


def check_closest(b, v, t, rays, what, ref=None):
    rt, rp, rb = ref if ref is not None else mesh_ref.closest(v, t, rays)
    out = b.trace_ex(rays, want=("t", "prim", "bary"))
    gt, gp, gb = out["t"], out["prim"], out["bary"]
    bad = np.flatnonzero((gt > 0) != (rt > 0))
    assert bad.size == 0, "%s: hit/miss differs on rays %s: gpu %s ref %s" % (what, bad[:5], gt[bad[:5]], rt[bad[:5]])
    assert np.array_equal(gt.view(np.uint32), rt.view(np.uint32)), "%s: t not bit-equal on %d rays" % (what, int((gt != rt).sum()))
    assert np.array_equal(gp, rp), "%s: prim differs on %d rays, first %s" % (what, int((gp != rp).sum()), np.flatnonzero(gp != rp)[:5])
    assert np.array_equal(gb.view(np.uint32), rb.view(np.uint32)), "%s: bary not bit-equal" % what
    return rt, rp


@pytest.mark.parametrize("name,nsample", [("cube", None), ("rotcube", None), ("floor", None), ("adversarial", None), ("blob70k", 1500),
                                          ("soup100k", 1500), ("atrium262k", 1000)])
def test_bvh_trace_vs_brute_force(gpu, name, nsample):
    v, t = scene(name)
    mesh = gpu.Mesh.from_arrays(v, t)
    bvhs = [mesh.bvh(max_leaf=m) for m in LEAF_SIZES]
    fams = ray_families(v, t, 4000 if nsample is None else nsample, 3)
    rng = np.random.default_rng(17)
    for fam, rays in fams.items():
        if nsample is not None and len(rays) > nsample:
            rays = rays[np.sort(rng.choice(len(rays), nsample, replace=False))]
        ref = mesh_ref.closest(v, t, rays)
        if fam in ("random", "vertex"):
            assert (ref[0] > 0).mean() > 0.02, fam
        for m, b in zip(LEAF_SIZES, bvhs):
            check_closest(b, v, t, rays, "%s max_leaf=%d %s" % (name, m, fam), ref)
        t1, p1, nh = bvhs[0].trace(rays)
        assert np.array_equal(t1, ref[0]) and np.array_equal(p1, ref[1]) and nh == int((ref[0] > 0).sum())


def test_bvh_trace_extended_outputs(gpu):
    v, t = floor_scene()
    b = gpu.Mesh.from_arrays(v, t).bvh()
    gi, vs = mesh_gi(v)
    rays = np.concatenate([vx_scenes.random_rays(3000, gi["bmin"], gi["bmax"], seed=5), inside_rays(gi, vs, 2000, 6), grazing_floor_rays(1000, 7)])
    rt, rp, rb = mesh_ref.closest(v, t, rays)
    out = b.trace_ex(rays, want=("t", "prim", "normal", "bary"))
    assert np.array_equal(out["t"], rt) and np.array_equal(out["prim"], rp) and np.array_equal(out["bary"], rb)
    assert np.abs(out["normal"] - mesh_ref.normals(v, t, rp)).max() <= 1e-6
    assert not out["normal"][rp == mesh_ref.MISS].any() and not out["bary"][rp == mesh_ref.MISS].any()
    tpr = np.random.default_rng(3).uniform(0.0, 8.0, len(rays)).astype(np.float32)
    sh = b.trace_ex(rays, any_hit=True, want=("shadowed", "t"))
    assert np.array_equal(sh["shadowed"], mesh_ref.any_hit(v, t, rays))
    assert np.all(sh["t"][sh["shadowed"] == 1] > 0)
    sh = b.trace_ex(rays, tmax_per_ray=tpr, any_hit=True, want=("shadowed",))["shadowed"]
    assert np.array_equal(sh, mesh_ref.any_hit(v, t, rays, tmax_per_ray=tpr))
    assert 0 < sh.sum() < len(rays)
    cl = b.trace_ex(rays, tmax_per_ray=tpr, want=("t", "prim", "bary"))
    et, ep, eb = mesh_ref.closest(v, t, rays, tmax_per_ray=tpr)
    assert np.array_equal(cl["t"], et) and np.array_equal(cl["prim"], ep) and np.array_equal(cl["bary"], eb)
    # the argument rules of vx_trace_ex*
    for want in (("prim",), ("normal",), ("bary",)):
        with pytest.raises(gpu.VxError) as e:
            b.trace_ex(rays, any_hit=True, want=want)
        assert e.value.status == INVALID_ARG


def test_bvh_trace_camera(gpu):
    v, t = floor_scene()
    b = gpu.Mesh.from_arrays(v, t).bvh()
    vi, pi = vx_scenes.camera_matrices()
    W, H = 160, 90
    ct = b.trace_ex(camera=(vi, pi, W, H), want=("t", "prim", "bary"))
    rays = oracle.primary_rays(vi, pi, W, H)
    rt, rp, rb = mesh_ref.closest(v, t, rays)
    assert (rt > 0).mean() > 0.1
    same = (ct["t"] == rt) & (ct["prim"] == rp)
    assert same.mean() > 0.999
    bt = b.trace_ex(rays, want=("t", "prim", "bary"))   # the restated rays by ray buffer: bit-equal
    assert np.array_equal(bt["t"], rt) and np.array_equal(bt["prim"], rp) and np.array_equal(bt["bary"], rb)


def test_bvh_trace_device_compacted_hits(gpu):
    import torch
    v, t = vx_scenes.scene("blob70k")
    b = gpu.Mesh.from_arrays(v, t).bvh()
    rays = vx_scenes.random_rays(100_000, v.min(0), v.max(0), seed=8)
    ht, hp, hn = b.trace(rays)
    dr = torch.from_numpy(rays).cuda()
    dt = torch.empty(len(rays), dtype=torch.float32, device="cuda")
    dp = torch.empty(len(rays), dtype=torch.int32, device="cuda")
    dbar = torch.empty(2 * len(rays), dtype=torch.float32, device="cuda")
    dh = torch.zeros(len(rays) * 3, dtype=torch.int32, device="cuda")
    dn = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.trace_device(dr.data_ptr(), len(rays), dt.data_ptr(), dp.data_ptr(), dh.data_ptr(), dn.data_ptr(), bary_ptr=dbar.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dt.cpu().numpy(), ht) and np.array_equal(dp.cpu().numpy().view(np.uint32), hp)
    hb = b.trace_ex(rays, want=("bary",))["bary"]
    assert np.array_equal(dbar.cpu().numpy().reshape(-1, 2), hb)
    nh = int(dn.cpu().item())
    assert nh == hn and nh > 1000
    hits = dh.cpu().numpy().view(gpu.HIT)[:nh]
    got = np.sort(hits, order=("ray",))
    idx = np.flatnonzero(ht > 0)
    assert np.array_equal(got["ray"], idx) and np.array_equal(got["prim"], hp[idx]) and np.array_equal(got["t"], ht[idx])
    dn.fill_(7)
    b.trace_device(dr.data_ptr(), len(rays), None, None, dh.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    assert int(dn.cpu().item()) == hn


def check_structure(b, v, t):
    nodes = b.nodes()
    lt = b.leaf_triangles().astype(np.int64)
    n = len(t)
    assert len(nodes) == b.num_nodes and b.num_triangles == n
    assert np.array_equal(np.sort(lt), np.arange(n))                   # leaf order is a permutation of the triangles
    is_leaf = (nodes["b"] & gpu_leaf()) != 0
    cnt = (nodes["b"] & ~np.uint32(gpu_leaf())).astype(np.int64)
    cover = np.zeros(n, np.int64)
    for a, c in zip(nodes["a"][is_leaf].astype(np.int64), cnt[is_leaf]):
        assert c >= 1
        cover[a:a + c] += 1
    assert np.all(cover == 1)                                          # every triangle in exactly one leaf
    tri_v = v[t[lt]]                                                   # [n, 3, 3] in leaf order
    tmn, tmx = tri_v.min(axis=1), tri_v.max(axis=1)
    # bounds bottom-up: leaves from their triangles, interior nodes from their children (= the exact min / max below, by induction)
    depth = np.full(len(nodes), -1, np.int64)
    depth[0] = 0
    order = [0]
    seen = np.zeros(len(nodes), np.int64)
    seen[0] = 1
    i = 0
    while i < len(order):
        k = order[i]
        i += 1
        if not is_leaf[k]:
            for c in (int(nodes["a"][k]), int(nodes["b"][k])):
                seen[c] += 1
                depth[c] = depth[k] + 1
                order.append(c)
    assert np.all(seen == 1)                                           # a tree: every node reached exactly once from the root
    assert depth.max() <= min(b.height, 62)
    mn, mx = np.zeros((len(nodes), 3), np.float32), np.zeros((len(nodes), 3), np.float32)
    for k in reversed(order):
        if is_leaf[k]:
            a, c = int(nodes["a"][k]), int(cnt[k])
            mn[k], mx[k] = tmn[a:a + c].min(axis=0), tmx[a:a + c].max(axis=0)
        else:
            l, r = int(nodes["a"][k]), int(nodes["b"][k])
            mn[k], mx[k] = np.minimum(mn[l], mn[r]), np.maximum(mx[l], mx[r])
    assert np.array_equal(nodes["mn"], mn) and np.array_equal(nodes["mx"], mx)
    rmn, rmx = b.root_bounds()
    assert np.array_equal(rmn, v[t].reshape(-1, 3).min(0)) and np.array_equal(rmx, v[t].reshape(-1, 3).max(0))
    return depth.max()


def gpu_leaf():
    import voxhip
    return voxhip.BVH_LEAF


@pytest.mark.parametrize("m", [1, 4, 16, 0])
def test_bvh_structure_small(gpu, m):
    v, t = vx_scenes.scene("adversarial")
    check_structure(gpu.Mesh.from_arrays(v, t).bvh(max_leaf=m), v, t)


def test_bvh_ill_conditioned_count(gpu):
    """the side list holds the slivers and collinear triangles, and only those"""
    v, t = vx_scenes.scene("adversarial")
    e1, e2 = (v[t[:, 1]] - v[t[:, 0]]).astype(np.float64), (v[t[:, 2]] - v[t[:, 0]]).astype(np.float64)
    c = np.cross(e1, e2)
    l1, l2 = (e1 * e1).sum(1), (e2 * e2).sum(1)
    thin = (l1 > 0) & (l2 > 0) & ((c * c).sum(1) <= 2.0 ** -20 * l1 * l2)
    assert thin.sum() > 50
    assert gpu.Mesh.from_arrays(v, t).bvh().num_ill_conditioned == int(thin.sum())
    cv, ct = vx_scenes.scene("rotcube")
    assert gpu.Mesh.from_arrays(cv, ct).bvh().num_ill_conditioned == 0


def test_bvh_structure_soup_2m(gpu):
    v, t = vx_scenes.soup(2_000_000)
    b = gpu.Mesh.from_arrays(v, t).bvh()
    d = check_structure(b, v, t)
    assert d >= 15
    rays = vx_scenes.random_rays(120, v.min(0), v.max(0), seed=9)
    check_closest(b, v, t, rays, "soup 2M")


def test_bvh_build_into_steady_state(gpu):
    import torch
    v2, t2 = vx_scenes.scene("blob70k")
    dv = torch.from_numpy(v2.copy()).cuda()
    di = torch.from_numpy(t2.copy()).cuda()
    torch.cuda.synchronize()
    mesh = gpu.Mesh.from_device(dv.data_ptr(), len(v2), di.data_ptr(), len(t2), keep=(dv, di))
    b = mesh.bvh()
    ptr, nn = b.nodes_device_ptr(), b.num_nodes
    rays = vx_scenes.random_rays(20_000, v2.min(0) - 0.5, v2.max(0) + 0.5, seed=4)
    # move the vertices in place, rebuild into the same handle
    dv.mul_(1.25).add_(torch.tensor([0.3, -0.2, 0.1], device="cuda"))
    torch.cuda.synchronize()
    allocs = gpu.device_allocations()
    b.build_into(mesh)
    assert gpu.device_allocations() == allocs          # no device block of the handle (BVH or build scratch) was requested again
    assert b.nodes_device_ptr() == ptr and b.num_nodes == nn
    fresh = mesh.bvh()
    got = b.trace_ex(rays, want=("t", "prim", "bary"))
    exp = fresh.trace_ex(rays, want=("t", "prim", "bary"))
    assert all(np.array_equal(got[k], exp[k]) for k in got)
    assert np.array_equal(b.nodes(), fresh.nodes())
    vm = dv.cpu().numpy()
    sel = np.random.default_rng(2).choice(len(rays), 300, replace=False)
    rt, rp, rb = mesh_ref.closest(vm, t2, rays[sel])
    assert np.array_equal(got["t"][sel], rt) and np.array_equal(got["prim"][sel], rp)
    # the mesh may go away: the BVH holds its own vertices
    mesh.free()
    del dv, di
    torch.cuda.synchronize()
    again = b.trace_ex(rays, want=("t", "prim", "bary"))
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_bvh_edges(gpu):
    import ctypes as C
    import torch
    empty = gpu.Mesh.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    b = empty.bvh()
    assert b.num_triangles == 0 and b.num_nodes == 0 and len(b.nodes()) == 0
    rays = vx_scenes.random_rays(500, np.float32([-1, -1, -1]), np.float32([1, 1, 1]), seed=1)
    out = b.trace_ex(rays, want=("t", "prim", "bary", "normal"))
    assert np.all(out["t"] == -1.0) and np.all(out["prim"] == 0xFFFFFFFF) and not out["bary"].any() and not out["normal"].any()
    assert not b.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"].any()
    # one triangle
    v1 = np.float32([[-1, -1, 0], [1, -1, 0], [0, 1, 0]])
    t1 = np.int32([[0, 1, 2]])
    b1 = gpu.Mesh.from_arrays(v1, t1).bvh()
    assert b1.num_nodes == 1
    check_closest(b1, v1, t1, rays, "one triangle")
    tt, pp, nh = b1.trace(np.zeros((0, 6), np.float32))
    assert nh == 0 and len(tt) == 0
    # a borrowed device mesh with an index out of range: VX_ERR_INVALID_ARG, no fault, the device stays usable
    dv = torch.from_numpy(v1.copy()).cuda()
    di = torch.from_numpy(np.int32([[0, 1, 2], [0, 3, 1]])).cuda()
    torch.cuda.synchronize()
    bad = gpu.Mesh.from_device(dv.data_ptr(), 3, di.data_ptr(), 2, keep=(dv, di))
    with pytest.raises(gpu.VxError) as e:
        bad.bvh()
    assert e.value.status == INVALID_ARG and "index" in e.value.message
    with pytest.raises(gpu.VxError) as e:
        b1.build_into(bad)
    assert e.value.status == INVALID_ARG
    assert b1.num_triangles == 0 and np.all(b1.trace(rays)[0] == -1.0)     # a failed rebuild leaves an empty BVH
    b1.build_into(gpu.Mesh.from_arrays(v1, t1))
    check_closest(b1, v1, t1, rays, "rebuilt")
    # the hit list is a device-side output
    a = gpu.BvhTraceArgs()
    r = np.ascontiguousarray(rays)
    tb = np.zeros(len(r), np.float32)
    hits = np.zeros(3 * len(r), np.int32)
    nhb = np.zeros(1, np.uint64)
    a.base.rays, a.base.num_rays, a.base.t, a.base.hits, a.base.num_hits = r.ctypes.data, len(r), tb.ctypes.data, hits.ctypes.data, nhb.ctypes.data
    assert gpu.lib().vx_bvh_trace_ex(b1.h, C.byref(a)) == UNSUPPORTED
    # any_hit with the hit list on the device variant: every pointer a device pointer, so that nothing could fault if a kernel ran
    dr = torch.from_numpy(r).cuda()
    dt = torch.empty(len(r), dtype=torch.float32, device="cuda")
    dh = torch.zeros(3 * len(r), dtype=torch.int32, device="cuda")
    dn = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d = gpu.BvhTraceArgs()
    d.base.rays, d.base.num_rays, d.base.t, d.base.hits, d.base.num_hits = dr.data_ptr(), len(r), dt.data_ptr(), dh.data_ptr(), dn.data_ptr()
    d.base.any_hit = 1
    assert gpu.lib().vx_bvh_trace_ex_device(b1.h, C.byref(d)) == INVALID_ARG
    d.base.hits, d.base.num_hits, d.bary = None, None, dt.data_ptr()
    assert gpu.lib().vx_bvh_trace_ex_device(b1.h, C.byref(d)) == INVALID_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,cells", [("blob70k", 256), ("atrium262k", 512)])
def test_bvh_voxelizer_conservative(gpu, name, cells):
    """A ray that meets a triangle at t_tri also meets an occupied voxel of the Bool grid no later."""
    v, t = vx_scenes.scene(name)
    ext = np.float32((v.max(0) - v.min(0)).max())
    vs = np.float32(ext / np.float32(cells))
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, vs)
    assert max(g.describe()["dim"]) == cells
    d = g.describe()
    rays = vx_scenes.random_rays(100_000, d["bbox_min"], d["bbox_max"], seed=12)   # origins outside the grid
    tt, _, _ = mesh.bvh().trace(rays)
    tv, _, _ = g.trace(rays)
    h = tt > 0
    assert h.mean() > 0.05
    ok = (tv[h] > 0) & (tv[h] <= tt[h] * np.float32(1 + 1e-5) + np.float32(1e-6))
    bad = np.flatnonzero(h)[~ok]
    assert bad.size == 0, "%d rays meet a triangle before any voxel, first %s: t_tri %s t_vox %s" % (bad.size, bad[:3], tt[bad[:3]], tv[bad[:3]])


def run_cli(args):
    exe = os.path.join(PKG, "voxilizer")
    return subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


def test_cli_mesh_behind_camera_is_invisible(gpu, tmp_path):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    obj, tri = tmp_path / "c.obj", tmp_path / "behind.obj"
    vx_scenes.write_obj(str(obj), v, t)
    eye = np.float32([6.16636, 2.42256, -3.15471])
    back = eye + (eye - np.float32([0.0, 1.0, 0.0])) * 2.0            # behind the camera, off every shadow ray to the light
    vx_scenes.write_obj(str(tri), np.float32([back, back + [0.5, 0, 0], back + [0, 0.5, 0]]), np.int32([[0, 1, 2]]))
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    r0 = run_cli([str(obj), "0.05", "--render", str(a), "--size", "160x90"])
    r1 = run_cli([str(obj), "0.05", "--render", str(b), "--size", "160x90", "--mesh", str(tri)])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout + r1.stdout
    assert open(a, "rb").read() == open(b, "rb").read()
    assert ", 0 hit a triangle" in r1.stdout and "hit a triangle" not in r0.stdout
    r = run_cli([str(obj), "0.05", "--mesh", str(tri)])
    assert r.returncode != 0 and "--mesh needs --render" in r.stdout
    for extra in (["--grid", "aabbstruct"], ["--grid", "vec"], ["--bench", "2"]):
        r = run_cli([str(obj), "0.05", "--render", str(b), "--mesh", str(tri)] + extra)
        assert r.returncode != 0 and "--mesh renders with --grid bool or octree only" in r.stdout, extra


@pytest.mark.parametrize("grid", ["bool", "octree"])
def test_cli_mesh_floor_count_matches_api(gpu, tmp_path, grid):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    fv = np.float32([[-6, -0.8, -6], [6, -0.8, -6], [6, -0.8, 6], [-6, -0.8, 6]])
    ft = np.int32([[0, 1, 2], [0, 2, 3]])
    obj, floor = tmp_path / "c.obj", tmp_path / "floor.obj"
    vx_scenes.write_obj(str(obj), v, t)
    vx_scenes.write_obj(str(floor), fv, ft)
    W, H = 160, 90
    ppm, cam = tmp_path / "o.ppm", tmp_path / "cam.bin"
    r = run_cli([str(obj), "0.05", "--grid", grid, "--render", str(ppm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam), "--mesh", str(floor)])
    assert r.returncode == 0, r.stdout
    cm = np.fromfile(cam, np.float32)
    camera = (cm[:16], cm[16:], W, H)
    mesh = gpu.Mesh.from_arrays(v, t)
    vox = gpu.Grid.voxelize(mesh, np.float32(0.05)) if grid == "bool" else gpu.Octree(mesh, np.float32(0.05))
    vt = vox.trace_ex(camera=camera, want=("t",))["t"]
    mt = gpu.Mesh.from_arrays(fv, ft).bvh().trace_ex(camera=camera, want=("t",))["t"]
    tri = (mt > 0) & ~((vt > 0) & (vt <= mt))                          # the closer hit; the voxel on equal t
    nvox = int(((vt > 0) & ~tri).sum())
    assert tri.sum() > 100 and nvox > 100
    assert ("%d hit a triangle" % int(tri.sum())) in r.stdout, r.stdout
    raw = open(ppm, "rb").read()
    img = np.frombuffer(raw[len(b"P6\n%d %d\n255\n" % (W, H)):], np.uint8).reshape(H * W, 3)
    assert len(np.unique(img[tri], axis=0)) > 3                        # the floor is lit, and shadowed in places


# ---- the --mesh picture, restated: voxilizer.cpp's render() in float32 numpy over the Python API's ray queries ----------------------------
F = np.float32
LIGHT, INTENSITY = F([10.0, 55.0, 8.0]), F(1000.0)     # hello_vulkan.h:86-88
DEFAULT_MAT = dict(ambient=F([0.1, 0.1, 0.1]), diffuse=F([1, 1, 0]), specular=F([1, 1, 1]), shininess=F(0), illum=0)   # MaterialObj{}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _norm(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def cli_dirs(vi, pi, W, H):
    """the host-side primary directions of render(): tg = norm(projInv * (ndc, 1, 1)), dir = viewInv * tg (as C++ evaluates them)"""
    i = np.arange(W * H)
    u = ((i % W).astype(F) + F(0.5)) / F(W)
    v = ((i // W).astype(F) + F(0.5)) / F(H)
    dx, dy = u * F(2) - F(1), v * F(2) - F(1)
    tg = _norm(np.stack([((pi[k] * dx + pi[4 + k] * dy) + pi[8 + k]) + pi[12 + k] for k in range(3)], 1))
    return np.stack([(vi[k] * tg[:, 0] + vi[4 + k] * tg[:, 1]) + vi[8 + k] * tg[:, 2] for k in range(3)], 1)


def _specular(mat, d, N, L):
    """computeSpecular, wavefront.glsl:32-48"""
    kSh = np.maximum(mat["shininess"], F(4))
    kE = (F(2) + kSh) / (F(2) * F(3.14159265))
    V = _norm(d * F(-1))
    I = L * F(-1)
    Rr = I - N * (F(2) * _dot(N, I))[:, None]
    sp = kE * np.power(np.maximum(_dot(V, Rr), F(0)), kSh)
    return mat["specular"][None, :] * sp[:, None]


def _shade(N, L, d, dist, mat, shadowed, att_unlit):
    li = INTENSITY / (dist * dist)
    dnl = np.maximum(_dot(N, L), F(0))
    diff = mat["diffuse"][None, :] * dnl[:, None]
    if mat["illum"] >= 1:
        diff = diff + mat["ambient"][None, :]
    lit = _dot(N, L) > 0
    att = np.where(lit & ~shadowed, F(1), np.where(lit, F(0.3), F(att_unlit)))
    spec = np.zeros_like(diff)
    if mat["illum"] >= 2:
        s = lit & ~shadowed
        spec[s] = _specular(mat, d[s], N[s], L[s])
    return (li * att)[:, None] * (diff + spec)


def restate_mesh_render(vox, bvh, v, t, mats, mat_ids, vi, pi, W, H):
    """-> (uint8[H*W, 3], tri mask, shadow masks (voxels, mesh)); vox: Grid or Octree"""
    n = W * H
    cam = (vi, pi, W, H)
    vo = vox.trace_ex(camera=cam, want=("t", "normal"))
    mo = bvh.trace_ex(camera=cam, want=("t", "prim", "normal", "bary"))
    vt, mt = vo["t"], mo["t"]
    tri = (mt > 0) & ~((vt > 0) & (vt <= mt))                           # the closer hit; the voxel on equal t
    d = cli_dirs(vi, pi, W, H)
    org = F(vi[12:15])
    ts = np.where(tri, mt, np.where(vt > 0, vt, F(0)))
    wp = org[None, :] + d * ts[:, None]
    pos = wp.copy()
    k = np.flatnonzero(tri)
    tv = v[t[mo["prim"][k].astype(np.int64)]]                            # [m, 3, 3]
    b1, b2 = mo["bary"][k, 0], mo["bary"][k, 1]
    b0 = (F(1) - b1) - b2
    pos[k] = (tv[:, 0] * b0[:, None] + tv[:, 1] * b1[:, None]) + tv[:, 2] * b2[:, None]   # rchit:67-68
    l = LIGHT[None, :] - pos
    dist = np.sqrt(_dot(l, l))
    L = l * (F(1) / dist)[:, None]
    rays = np.ascontiguousarray(np.concatenate([wp, L], 1).astype(F))
    sv = vox.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"].astype(bool)
    sm = bvh.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"].astype(bool)
    sh = sv | sm
    c = np.full((n, 3), F(0.8), F)                                       # rmiss:37
    h = (vt > 0) & ~tri                                                  # raytrace2.rchit with MaterialObj{}
    c[h] = _shade(vo["normal"][h], L[h], d[h], dist[h], DEFAULT_MAT, sh[h], 0.3)
    N = mo["normal"].copy()
    N[_dot(N, d) > 0] *= F(-1)                                           # the geometric normal, toward the ray
    mid = np.full(n, -1, np.int64) if mat_ids is None else mat_ids[np.minimum(mo["prim"], len(t) - 1).astype(np.int64)]
    for m in np.unique(mid[tri]):                                        # raytrace.rchit:49-143 per material
        s = tri & (mid == m)
        mat = DEFAULT_MAT if m < 0 else dict(ambient=F(mats[m]["ambient"]), diffuse=F(mats[m]["diffuse"]), specular=F(mats[m]["specular"]),
                                             shininess=F(mats[m]["shininess"]), illum=int(mats[m]["illum"]))
        c[s] = _shade(N[s], L[s], d[s], dist[s], mat, sh[s], 1.0)
    g = np.power(np.minimum(np.maximum(c, F(0)), F(1)), F(1.0) / F(2.2))  # post.frag:36
    return np.floor(g * F(255) + F(0.5)).astype(np.uint8), tri, sv, sm


def write_mesh_obj(path, with_mtl):
    """a floor under the cube and a small canopy above it, between the cube and the light (its shadow falls on the voxels); with_mtl:
    the floor carries a .mtl material with specular, the canopy none (MaterialObj{})"""
    fv = [[-6, -0.8, -6], [6, -0.8, -6], [6, -0.8, 6], [-6, -0.8, 6]]
    cv = [[-0.2, 4.0, -0.6], [1.2, 4.0, -0.6], [1.2, 4.0, 0.8], [-0.2, 4.0, 0.8]]
    lines = []
    if with_mtl:
        with open(os.path.join(os.path.dirname(path), "floor.mtl"), "w") as fh:
            fh.write("newmtl tiles\nKa 0.05 0.05 0.05\nKd 0.6 0.5 0.4\nKs 0.3 0.3 0.3\nNs 24\nillum 2\n")
        lines.append("mtllib floor.mtl")
    lines += ["v %g %g %g" % tuple(p) for p in fv + cv]
    lines += ["f 5 6 7", "f 5 7 8"]                                   # the canopy: before any usemtl, no material
    if with_mtl:
        lines.append("usemtl tiles")
    lines += ["f 1 2 3", "f 1 3 4"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("grid,with_mtl", [("bool", True), ("octree", False)])
def test_cli_mesh_shading_matches_restatement(gpu, tmp_path, grid, with_mtl):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    obj, mobj = tmp_path / "c.obj", tmp_path / "scene.obj"
    vx_scenes.write_obj(str(obj), v, t)
    write_mesh_obj(str(mobj), with_mtl)
    W, H = 320, 180
    ppm, cam = tmp_path / "o.ppm", tmp_path / "cam.bin"
    r = run_cli([str(obj), "0.05", "--grid", grid, "--render", str(ppm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam), "--mesh", str(mobj)])
    assert r.returncode == 0, r.stdout
    cm = np.fromfile(cam, np.float32)
    mesh = gpu.Mesh.from_arrays(v, t)
    vox = gpu.Grid.voxelize(mesh, np.float32(0.05)) if grid == "bool" else gpu.Octree(mesh, np.float32(0.05))
    model = gpu.Mesh.load_obj(str(mobj))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    assert (len(mats) == 1 and ids is not None and (ids == -1).sum() == 2) if with_mtl else (len(mats) == 0 and ids is None)
    ref, tri, sv, sm = restate_mesh_render(vox, model.bvh(), mv, mtris, mats, ids, cm[:16], cm[16:], W, H)
    raw = open(ppm, "rb").read()
    img = np.frombuffer(raw[len(b"P6\n%d %d\n255\n" % (W, H)):], np.uint8).reshape(H * W, 3)
    # the cases the restatement has to cover, each with enough pixels: floor in the cube's shadow, lit floor, and voxels lit only
    # because nothing but the canopy's triangles stand between them and the light (shadowed by the mesh, not by other voxels)
    floor_shadow = tri & sv
    vox_by_mesh = (~tri) & sm & ~sv
    assert floor_shadow.sum() >= 20 and (tri & ~sv & ~sm).sum() >= 200 and vox_by_mesh.sum() >= 20, (floor_shadow.sum(), vox_by_mesh.sum())
    diff = np.abs(img.astype(np.int16) - ref.astype(np.int16)).max(axis=1)
    bad = np.flatnonzero(diff > 1)
    assert bad.size == 0, "%d pixels differ by more than 1 LSB, first %s: cli %s restated %s" % (bad.size, bad[:3], img[bad[:3]], ref[bad[:3]])
    # and a seeded sample drawn from each case is the picture's own, not the miss colour
    rng = np.random.default_rng(21)
    for m in (floor_shadow, vox_by_mesh, tri & ~sv & ~sm):
        s = rng.choice(np.flatnonzero(m), 20, replace=False)
        assert np.all(np.abs(img[s].astype(np.int16) - ref[s].astype(np.int16)) <= 1) and (img[s] != 204).any()
