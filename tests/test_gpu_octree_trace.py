"""GPU tests of the ray queries on the octree (vx_octree_trace*, k_octree_trace): first hit, shadow query, cube normals, camera rays and the
compacted hit list over the list vx_octree_aabbs() returns, against the CPU oracle's list-generic brute force -- t and prim bit-equal."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import vx_scenes
from test_gpu_parity import axis_rays, corner_rays, inside_rays, long_thin_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
LEAF_SIZES = [1, 16, 64, 100]          # direct node-array form (<= 64) and the level-by-level form (> 64)
INVALID_ARG, CAPACITY, UNSUPPORTED = 1, 8, 9


def zero_component_rays(gi, vs, n, seed):
    """Directions with exact zero components (1/d = +-inf: 0 * inf = NaN in hitAabb), origins on and between lattice planes."""
    rng = np.random.default_rng(seed)
    dim = np.array(gi["dim"])
    bmin = gi["bmin"].astype(np.float64)
    k = rng.integers(0, dim + 1, size=(n, 3)).astype(np.float64) + rng.choice([0.0, 0.5, 0.25], size=(n, 3))
    o = bmin + k * vs
    d = rng.normal(size=(n, 3))
    nz = rng.integers(1, 3, n)                           # one or two zero components
    for i in range(n):
        d[i, rng.choice(3, nz[i], replace=False)] = 0.0
    d = np.where((d == 0.0) & (rng.random((n, 3)) < 0.5), -0.0, d)   # both signs of zero
    back = bmin + dim * vs * rng.choice([-0.5, 1.5], n)[:, None]
    for i in range(n):                                   # start outside along a non-zero axis half of the time
        if i % 2:
            ax = int(np.flatnonzero(d[i] != 0)[0])
            o[i, ax] = back[i, ax]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1).astype(np.float32))


def ray_families(gi, vs, n, seed):
    return {"random": vx_scenes.random_rays(n, gi["bmin"], gi["bmax"], seed=seed), "corner": corner_rays(gi, vs, n // 2, seed + 1),
            "axis": axis_rays(gi, vs, 1500, seed + 2), "zero": zero_component_rays(gi, vs, 1500, seed + 3),
            "inside": inside_rays(gi, vs, n // 2, seed + 4)}


def check_against(o, oa, rays, ot, op, what=""):
    t, p, nh = o.trace(rays)
    bad = np.flatnonzero((t > 0) != (ot > 0))
    assert bad.size == 0, "%s: hit/miss differs on rays %s: gpu %s oracle %s" % (what, bad[:5], t[bad[:5]], ot[bad[:5]])
    assert np.array_equal(t.view(np.uint32), ot.view(np.uint32)), "%s: t not bit-equal on %d rays" % (what, int((t != ot).sum()))
    assert np.array_equal(p, op), "%s: prim differs on %d rays" % (what, int((p != op).sum()))
    assert nh == int((ot > 0).sum())
    return t, p


@pytest.mark.parametrize("name,vs", [("cube", 0.25), ("cube", 0.0625), ("rotcube", 0.09), ("adversarial", 0.0625), ("adversarial", 0.1),
                                     ("soup2000", 0.02), ("blob70k", 2.0 / 64)])
def test_octree_trace_vs_brute_force(gpu, name, vs):
    v, t = vx_scenes.scene(name)
    vs = np.float32(vs)
    mesh = gpu.Mesh.from_arrays(v, t)
    trees = [gpu.Octree(mesh, vs, max_items=m) for m in LEAF_SIZES]
    oa = trees[0].aabbs()
    for o in trees[1:]:
        assert o.aabbs().tobytes() == oa.tobytes()       # the list does not depend on the leaf size
    gi = oracle.build_bool(v, t, vs)[2]
    n = 6000 if len(oa) < 20000 else 3000
    for fam, rays in ray_families(gi, float(vs), n, 2).items():
        ot, op = oracle.trace_brute(oa, rays)
        if fam == "random":
            assert (ot > 0).mean() > 0.02
        for m, o in zip(LEAF_SIZES, trees):
            check_against(o, oa, rays, ot, op, "%s max_items=%d %s" % (name, m, fam))


def test_octree_trace_extended_outputs(gpu):
    v, t = vx_scenes.scene("rotcube")
    vs = np.float32(0.05)
    mesh = gpu.Mesh.from_arrays(v, t)
    gi = oracle.build_bool(v, t, vs)[2]
    rays = np.concatenate([vx_scenes.random_rays(4000, gi["bmin"], gi["bmax"], seed=5), inside_rays(gi, float(vs), 2000, 6)])
    tpr = np.random.default_rng(3).uniform(0.0, 3.0, len(rays)).astype(np.float32)
    for m in (16, 100):
        o = gpu.Octree(mesh, vs, max_items=m)
        oa = o.aabbs()
        ot, op = oracle.trace_brute(oa, rays)
        out = o.trace_ex(rays, want=("t", "prim", "normal"))
        assert np.array_equal(out["t"], ot) and np.array_equal(out["prim"], op)
        assert np.array_equal(out["normal"], oracle.cube_normals(oa, op, rays, ot))
        sh = o.trace_ex(rays, any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(sh, oracle.trace_any_brute(oa, rays))
        sh = o.trace_ex(rays, tmax_per_ray=tpr, any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(sh, oracle.trace_any_brute(oa, rays, tmax_per_ray=tpr))
        assert 0 < sh.sum() < len(rays)
        # per-ray tMax on the closest hit: the brute force with that ray's own tmax
        cl = o.trace_ex(rays, tmax_per_ray=tpr, want=("t", "prim"))
        for k in range(0, len(rays), 97):
            et, ep = oracle.trace_brute(oa, rays[k:k + 1], tmax=float(tpr[k]))
            assert cl["t"][k] == et[0] and cl["prim"][k] == ep[0]
        hit = cl["t"] > 0
        assert np.all(cl["t"][hit] <= tpr[hit]) and np.all(ot[hit] <= cl["t"][hit])


def test_octree_trace_camera_matches_bool_grid(gpu):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    vs = np.float32(0.05)
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, vs)
    o = gpu.Octree(mesh, vs)
    assert np.unique(o.aabbs()).tobytes() == np.unique(g.aabbs()).tobytes()   # the same set of distinct boxes
    vi, pi = vx_scenes.camera_matrices()
    W, H = 160, 90
    ct = o.trace_ex(camera=(vi, pi, W, H), want=("t", "prim", "normal"))
    gt = g.trace_ex(camera=(vi, pi, W, H), want=("t",))["t"]
    assert (gt > 0).mean() > 0.02
    assert np.array_equal(ct["t"].view(np.uint32), gt.view(np.uint32))
    # the camera rays themselves are the generator's: the same result from the oracle's restatement of them, traced by ray buffer
    rays = oracle.primary_rays(vi, pi, W, H)
    rt = o.trace_ex(rays, want=("t", "prim"))
    same = rt["t"] == ct["t"]
    assert same.mean() > 0.999


def test_octree_trace_device_compacted_hits(gpu):
    import torch
    v, t = vx_scenes.scene("blob70k")
    vs = np.float32(2.0 / 64)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), vs)
    gi = oracle.build_bool(v, t, vs)[2]
    rays = vx_scenes.random_rays(100_000, gi["bmin"], gi["bmax"], seed=8)
    ht, hp, hn = o.trace(rays)
    dr = torch.from_numpy(rays).cuda()
    dt = torch.empty(len(rays), dtype=torch.float32, device="cuda")
    dp = torch.empty(len(rays), dtype=torch.int32, device="cuda")
    dh = torch.zeros(len(rays) * 3, dtype=torch.int32, device="cuda")
    dn = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    o.trace_device(dr.data_ptr(), len(rays), dt.data_ptr(), dp.data_ptr(), dh.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dt.cpu().numpy(), ht) and np.array_equal(dp.cpu().numpy().view(np.uint32), hp)
    nh = int(dn.cpu().item())
    assert nh == hn and nh > 1000
    hits = dh.cpu().numpy().view(gpu.HIT)[:nh]
    got = np.sort(hits, order=("ray",))
    idx = np.flatnonzero(ht > 0)
    assert np.array_equal(got["ray"], idx) and np.array_equal(got["prim"], hp[idx]) and np.array_equal(got["t"], ht[idx])
    # without t / prim outputs: the list alone
    dn.fill_(7)
    o.trace_device(dr.data_ptr(), len(rays), None, None, dh.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    assert int(dn.cpu().item()) == hn


def test_octree_trace_atrium_512(gpu):
    """BASELINE configs[2] scale: atrium262k at exactly 512^3, 1M random rays; the octree's t is the Bool grid's on every ray."""
    v, t = vx_scenes.scene("atrium262k")
    vs = np.float32(32.0 / 512)
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, vs)
    assert g.describe()["dim"] == (512, 512, 512)
    o = gpu.Octree(mesh, vs)
    d = g.describe()
    rays = vx_scenes.random_rays(1_000_000, d["bbox_min"], d["bbox_max"], seed=2)
    gt, _, gn = g.trace(rays)
    tt, pp, nh = o.trace(rays)
    assert np.array_equal(tt.view(np.uint32), gt.view(np.uint32)) and nh == gn
    oa = o.aabbs()
    items = o.items()
    h = np.flatnonzero(tt > 0)
    assert np.all(pp[tt <= 0] == 0xFFFFFFFF)
    org, dr = rays[h, :3], rays[h, 3:]
    inv = np.float32(1.0) / dr
    b = oa[pp[h]]
    tb, tp = inv * (b["mn"] - org), inv * (b["mx"] - org)
    assert np.array_equal(np.minimum(tb, tp).max(axis=1).astype(np.float32), tt[h])  # hitAabb of the reported box
    ph = pp[h].astype(np.int64)
    assert np.all((ph == 0) | (items[np.maximum(ph - 1, 0)] != items[ph]))            # the first index of its run of equal codes
    sel = np.random.default_rng(11).choice(len(rays), 1000, replace=False)
    ot, op = oracle.trace_brute(oa, rays[sel])
    assert np.array_equal(tt[sel], ot) and np.array_equal(pp[sel], op)


def two_cluster_mesh(span=6000.0):
    """Two rotated cubes about 10 voxels across (voxel size 1) at opposite corners of a box of more than `span` cells per axis."""
    va, ta = vx_scenes.rotated_cube(half=5.0, offset=(8.0, 8.0, 8.0))
    vb, tb = vx_scenes.rotated_cube(half=5.0, angles=(0.11, 0.83, 0.47), offset=(span, span, span))
    return np.concatenate([va, vb]).astype(np.float32), np.concatenate([ta, tb + len(va)]).astype(np.int32)


def test_octree_trace_beyond_dense_cap(gpu):
    v, t = two_cluster_mesh()
    vs = np.float32(1.0)
    mesh = gpu.Mesh.from_arrays(v, t)
    with pytest.raises(gpu.VxError) as e:
        gpu.Grid.voxelize(mesh, vs)
    assert e.value.status == CAPACITY
    for m in (16, 100):
        o = gpu.Octree(mesh, vs, max_items=m)
        dim = np.ceil((v.max(0) - v.min(0)) / vs)
        assert dim.min() >= 6000 and np.prod(dim) > 2.0 ** 37 and dim.max() < 65536
        oa = o.aabbs()
        assert 100 < len(oa) < 100_000
        rng = np.random.default_rng(4)
        n = 3000
        src = v.min(0) + rng.uniform(0, 1, (n, 3)) * (v.max(0) - v.min(0))
        tgt = np.where(rng.random((n, 1)) < 0.5, np.array([8.0, 8.0, 8.0]), np.array([6000.0, 6000.0, 6000.0])) + rng.uniform(-6, 6, (n, 3))
        d = tgt - src
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        aimed = np.concatenate([src, d], axis=1).astype(np.float32)
        rays = np.concatenate([aimed, vx_scenes.random_rays(2000, v.min(0), v.max(0), seed=6)])
        ot, op = oracle.trace_brute(oa, rays)
        assert (ot[:n] > 0).mean() > 0.3
        check_against(o, oa, rays, ot, op, "two clusters max_items=%d" % m)


def test_octree_trace_axis_above_65535(gpu):
    """100 000 x 8 x 8 cells: the traced boxes are the octree's own list, with the reference's low-16-bit Morton aliasing."""
    v, t = long_thin_mesh()
    vs = np.float32(1.0)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), vs)
    oa = o.aabbs()
    assert oa["mx"][:, 0].max() <= 65536.0 + 1.0                                    # aliased: no box beyond x = 65536
    rng = np.random.default_rng(3)
    n = 1500
    x0 = rng.uniform(0.0, 100_000.0, n)                                            # across the aliasing boundary at x = 65536
    src = np.stack([x0, rng.choice([-6.0, 14.0], n), rng.uniform(0.0, 8.0, n)], 1)
    tgt = np.stack([x0 + rng.uniform(-30.0, 30.0, n), rng.uniform(0.0, 8.0, n), rng.uniform(0.0, 8.0, n)], 1)
    d = tgt - src
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    along = np.concatenate([np.stack([rng.uniform(0, 100_000.0, 500), rng.uniform(0, 8, 500), rng.uniform(0, 8, 500)], 1),
                            np.tile([[1.0, 0.0, 0.0]], (500, 1)) * rng.choice([-1.0, 1.0], (500, 1))], 1)   # inside, along x
    rays = np.concatenate([np.concatenate([src, d], 1), along]).astype(np.float32)
    ot, op = oracle.trace_brute(oa, rays)
    assert (ot > 0).sum() > 300
    check_against(o, oa, rays, ot, op, "long thin")


def test_octree_trace_edges(gpu):
    # an empty mesh: every ray misses; zero rays
    empty = gpu.Mesh.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    o = gpu.Octree(empty, np.float32(0.1))
    rays = vx_scenes.random_rays(500, np.float32([-1, -1, -1]), np.float32([1, 1, 1]), seed=1)
    tt, pp, nh = o.trace(rays)
    assert nh == 0 and np.all(tt == -1.0) and np.all(pp == 0xFFFFFFFF)
    v, t = vx_scenes.scene("rotcube")
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), np.float32(0.09))
    tt, pp, nh = o.trace(np.zeros((0, 6), np.float32))
    assert nh == 0 and len(tt) == 0
    # every ray missing: pointing away from the mesh
    far = rays.copy()
    far[:, :3] = 50.0
    far[:, 3:] = np.abs(far[:, 3:]) + 0.1
    tt, pp, nh = o.trace(far)
    assert nh == 0 and np.all(tt == -1.0) and np.all(pp == 0xFFFFFFFF)
    sh = o.trace_ex(far, any_hit=True, want=("shadowed",))["shadowed"]
    assert not sh.any()
    # argument errors
    for want in (("prim",), ("normal",)):
        with pytest.raises(gpu.VxError) as e:
            o.trace_ex(rays, any_hit=True, want=want)
        assert e.value.status == INVALID_ARG
    import ctypes as C
    a = gpu.TraceArgs()
    r = np.ascontiguousarray(rays)
    tb = np.zeros(len(r), np.float32)
    hits = np.zeros(3 * len(r), np.int32)
    nhb = np.zeros(1, np.uint64)
    a.rays, a.num_rays, a.t, a.hits, a.num_hits = r.ctypes.data, len(r), tb.ctypes.data, hits.ctypes.data, nhb.ctypes.data
    assert gpu.lib().vx_octree_trace_ex(o.h, C.byref(a)) == UNSUPPORTED      # the hit list is a device-side output
    a.any_hit = 1
    assert gpu.lib().vx_octree_trace_ex_device(o.h, C.byref(a)) == INVALID_ARG
    assert gpu.lib().vx_octree_trace_ex_device(None, C.byref(a)) == INVALID_ARG
    assert gpu.lib().vx_octree_trace(None, r.ctypes.data, len(r), np.float32(0.001), np.float32(1e4), None, None, None) == INVALID_ARG


def test_cli_octree_render(gpu, tmp_path):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    obj = tmp_path / "c.obj"
    vx_scenes.write_obj(str(obj), v, t)
    W, H = 240, 135
    ppm, cam = tmp_path / "o.ppm", tmp_path / "cam.bin"
    exe = os.path.join(PKG, "voxilizer")
    r = subprocess.run([exe, str(obj), "0.05", "--grid", "octree", "--render", str(ppm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "rendered %dx%d" % (W, H) in r.stdout
    raw = open(ppm, "rb").read()
    hdr = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(hdr)
    img = np.frombuffer(raw[len(hdr):], np.uint8).reshape(H, W, 3)
    cm = np.fromfile(cam, np.float32)
    o = gpu.Octree(gpu.Mesh.from_arrays(v, t), np.float32(0.05))
    ref = oracle.shade_image(o.aabbs(), cm[:16], cm[16:], W, H)
    close = (np.abs(img.astype(np.int16) - ref.astype(np.int16)) <= 1).all(axis=2)
    assert close.mean() > 0.997, "only %.4f of the pixels within 1 LSB" % close.mean()
    assert (img != img[0, 0]).any(axis=2).mean() > 0.02                             # voxels in the picture, not only the miss colour
    r = subprocess.run([exe, str(obj), "0.05", "--grid", "octree", "--materials"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode != 0 and "materials" in r.stdout
