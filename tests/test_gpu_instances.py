"""GPU tests of the instanced scenes (vx_tlas_*, k_tlas_trace): t, instance, prim and bary bit-equal to the numpy brute force over every
(instance, triangle) pair of tests/instance_ref.py; the world-to-object matrices bit-equal to the pinned float64 formula; inactive
instances; updates from host and device arrays without allocation; BLAS rebuilds; 100k instances."""
import numpy as np
import pytest

import instance_ref
import vx_scenes

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF


def small_blob():
    return vx_scenes.blob(nlon=24, nlat=20)


def random_transforms(n, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        rot = instance_ref.random_rotation(rng)
        kind = k % 4
        if kind == 0:
            sc = np.full(3, rng.uniform(0.5, 2.0))
        elif kind == 1:
            sc = rng.uniform(0.3, 3.0, 3)
        elif kind == 2:
            sc = rng.uniform(0.5, 2.0, 3) * np.array([-1, 1, 1])   # mirrored: det < 0
        else:
            sc = rng.uniform(0.5, 2.0, 3)
        shear = rng.uniform(-0.6, 0.6) if kind == 3 else 0.0
        out.append(instance_ref.transform(rot, sc, shear, rng.uniform(-spread, spread, 3)))
    return np.asarray(out, np.float32)


def rays_around(n, lo, hi, seed):
    return vx_scenes.random_rays(n, np.float32(lo), np.float32(hi), seed=seed)


def grazing_axis_rays(n, seed, lo=-8.0, hi=8.0):
    """axis-aligned directions (zero components) and rays skimming y = 0 planes"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = np.zeros((n, 3), np.float32)
    ax = rng.integers(0, 3, n)
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    g = n // 2
    o[g:, 1] = 0.0
    d[g:] = rng.standard_normal((n - g, 3)).astype(np.float32)
    d[g:, 1] = 0.0
    return np.concatenate([o, d], axis=1).astype(np.float32)


def check(tl, meshes, inst, rays, what, tmax_per_ray=None):
    got = tl.trace_ex(rays, tmax_per_ray=tmax_per_ray, want=("t", "instance", "prim", "bary"))
    t, i, p, b = instance_ref.closest(meshes, inst, rays, tmax_per_ray=tmax_per_ray)
    for k, ref in (("t", t), ("instance", i), ("prim", p)):
        bad = np.nonzero(got[k].view(np.uint32) != ref.view(np.uint32))[0]
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:5]], ref[bad[:5]], got["instance"][bad[:5]], i[bad[:5]])
    assert np.array_equal(got["bary"].view(np.uint32), b.view(np.uint32)), what
    return t


def test_tlas_identity_matches_bvh(gpu, vx):
    v, t = vx_scenes.scene("atrium262k")
    mesh = vx.Mesh.from_arrays(v, t)
    b = vx.Bvh(mesh)
    tl = vx.Tlas([b], vx.instances([instance_ref.transform()]))
    assert tl.num_instances() == 1 and tl.num_nodes() == 1 and tl.height() == 0
    rays = vx_scenes.random_rays(1_000_000, v.min(0), v.max(0), seed=11)
    ref = b.trace_ex(rays, want=("t", "prim", "bary"))
    got = tl.trace_ex(rays, want=("t", "instance", "prim", "bary"))
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["prim"], ref["prim"])
    assert np.array_equal(got["bary"], ref["bary"])  # by value: a zero direction component may change sign through the transform
    assert np.array_equal(got["instance"], np.where(ref["t"] > 0, 0, MISS).astype(np.uint32))
    vi, pi = vx_scenes.camera_matrices(eye=(0.0, 4.0, 0.0), ctr=(10.0, 3.0, 5.0))
    cam = (vi, pi, 640, 360)
    ref = b.trace_ex(camera=cam, want=("t", "prim", "bary"))
    got = tl.trace_ex(camera=cam, want=("t", "prim", "bary"))
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)) and np.array_equal(got["prim"], ref["prim"])
    assert np.array_equal(got["bary"], ref["bary"])


@pytest.mark.parametrize("name", ["rotcube", "blob"])
def test_tlas_64_random_instances_vs_brute_force(gpu, vx, name):
    v, t = vx_scenes.scene("rotcube") if name == "rotcube" else small_blob()
    b = vx.Bvh(vx.Mesh.from_arrays(v, t))
    inst = instance_ref.make_instances(random_transforms(64, seed=3))
    tl = vx.Tlas([b], inst)
    rays = np.concatenate([rays_around(4000, -9, 9, 12), grazing_axis_rays(2000, 13)])
    check(tl, [(v, t)], inst, rays, name)
    w, _ = instance_ref.inverse(inst["transform"])
    assert np.array_equal(tl.world_to_object().view(np.uint32), w.view(np.uint32))
    nodes = tl.nodes()
    assert len(nodes) == 2 * 64 - 1
    leaves = nodes[(nodes["b"] & vx.BVH_LEAF) != 0]
    assert sorted(leaves["a"].tolist()) == list(range(64))


def test_tlas_shared_blas_duplicates_far_and_scaled(gpu, vx):
    cv, ct = vx_scenes.scene("rotcube")
    bv, bt = small_blob()
    fv = np.float32([[-4, 0, -4], [4, 0, -4], [4, 0, 4], [-4, 0, 4]])   # an axis-aligned floor on its box faces
    ft = np.int32([[0, 1, 2], [0, 2, 3]])
    meshes = [(cv, ct), (bv, bt), (fv, ft)]
    blas = [vx.Bvh(vx.Mesh.from_arrays(m[0], m[1])) for m in meshes]
    tr = list(random_transforms(24, seed=4))
    tr += [tr[0], tr[0], tr[5]]                                                   # coincident duplicates
    tr += [instance_ref.transform(offset=(1e4, 0, 0)), instance_ref.transform(scale=(1e-3,) * 3, offset=(1, 1, 1)),
           instance_ref.transform(scale=(1e3,) * 3, offset=(0, -3000, 0)), instance_ref.transform(), instance_ref.transform(offset=(0, -2, 0))]
    bl = [k % 2 for k in range(27)] + [0, 1, 1, 2, 2]
    inst = instance_ref.make_instances(tr, blas=bl)
    tl = vx.Tlas(blas, inst)
    rays = np.concatenate([rays_around(3000, -9, 9, 21), grazing_axis_rays(3000, 22)])
    far = rays_around(500, [1e4 - 2, -2, -2], [1e4 + 2, 2, 2], 23)
    tiny = rays_around(500, [0.998, 0.998, 0.998], [1.002, 1.002, 1.002], 24)
    check(tl, meshes, inst, np.concatenate([rays, far, tiny]), "mixed")
    tm = np.random.default_rng(5).uniform(0.0, 12.0, len(rays)).astype(np.float32)
    check(tl, meshes, inst, rays, "tmax_per_ray", tmax_per_ray=tm)
    sh = tl.trace_ex(rays, tmax_per_ray=tm, any_hit=True, want=("shadowed",))["shadowed"]
    assert np.array_equal(sh, instance_ref.any_hit(meshes, inst, rays, tmax_per_ray=tm))


def test_tlas_inactive_and_empty(gpu, vx):
    cv, ct = vx_scenes.scene("rotcube")
    b = vx.Bvh(vx.Mesh.from_arrays(cv, ct))
    e = vx.Bvh(vx.Mesh.from_arrays(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)))
    ident = instance_ref.transform()
    inst = instance_ref.make_instances([ident, instance_ref.transform(scale=(1, 0, 1)), ident, ident], blas=[0, 0, 1, 0], mask=[0, 0xFF, 0xFF, 0xFF])
    inst["mask"][3] = 0
    tl = vx.Tlas([b, e], inst)
    rays = rays_around(3000, -3, 3, 31)
    t, i, p, n = tl.trace(rays)
    assert n == 0 and (t == -1).all() and (i == MISS).all() and (p == MISS).all()
    tl.update(instance_ref.make_instances([], blas=[]))
    assert tl.num_instances() == 0 and tl.num_nodes() == 0
    t, i, p, n = tl.trace(rays)
    assert n == 0 and (i == MISS).all()


def test_tlas_updates_host_and_device(gpu, vx):
    import torch
    v, t = small_blob()
    b = vx.Bvh(vx.Mesh.from_arrays(v, t))
    inst = instance_ref.make_instances(random_transforms(40, seed=41))
    tl = vx.Tlas([b], inst)
    rays = rays_around(3000, -9, 9, 42)
    tl.trace(rays)
    for k in range(4):
        inst = instance_ref.make_instances(random_transforms(40, seed=50 + k))
        tl.update(inst)
        got = tl.trace_ex(rays, want=("t", "instance", "prim", "bary"))
        fresh = vx.Tlas([b], inst).trace_ex(rays, want=("t", "instance", "prim", "bary"))
        for key in got:
            assert np.array_equal(got[key], fresh[key]), (k, key)
    inst = instance_ref.make_instances(random_transforms(40, seed=60))
    dev = torch.from_numpy(inst.view(np.uint8).copy()).to("cuda")
    tl.update(device_ptr=dev, count=40)
    check(tl, [(v, t)], inst, rays, "device update")
    a1 = vx.lib().vx_device_allocations()
    for k in range(3):
        tl.update(instance_ref.make_instances(random_transforms(40, seed=70 + k)))
        tl.update(device_ptr=dev, count=40)
    torch.cuda.synchronize()
    assert vx.lib().vx_device_allocations() == a1
    # a device array that names a BLAS out of range / a singular transform: inactive, not an error
    bad = inst.copy()
    bad["blas"][0] = 7
    bad["transform"][1] = instance_ref.transform(scale=(0, 1, 1))
    dev2 = torch.from_numpy(bad.view(np.uint8).copy()).to("cuda")
    tl.update(device_ptr=dev2, count=40)
    check(tl, [(v, t)], bad, rays, "inactive by device update")


def test_tlas_blas_rebuild_then_update(gpu, vx):
    v, t = vx_scenes.scene("rotcube")
    mesh = vx.Mesh.from_arrays(v, t)
    b = vx.Bvh(mesh)
    inst = instance_ref.make_instances(random_transforms(16, seed=81))
    tl = vx.Tlas([b], inst)
    v2 = (v * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    b.build_into(vx.Mesh.from_arrays(v2, t))
    tl.update(inst)
    check(tl, [(v2, t)], inst, rays_around(3000, -9, 9, 82), "rebuilt BLAS")


def test_tlas_100k_instances(gpu, vx):
    v, t = vx_scenes.scene("rotcube")
    b = vx.Bvh(vx.Mesh.from_arrays(v, t))
    n = 100_000
    rng = np.random.default_rng(91)
    tr = np.zeros((n, 12), np.float32)
    s = rng.uniform(0.05, 0.2, n).astype(np.float32)
    tr[:, 0] = s; tr[:, 5] = s; tr[:, 10] = s
    tr[:, [3, 7, 11]] = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    inst = instance_ref.make_instances(tr)
    tl = vx.Tlas([b], inst)
    assert tl.num_nodes() == 2 * n - 1
    h = tl.height()
    assert 17 <= h <= 30 + 17, h
    rays = rays_around(16, -50, 50, 92)
    got = tl.trace_ex(rays, want=("t", "instance", "prim"))
    ref_t, ref_i, ref_p, _ = instance_ref.closest([(v, t)], inst, rays)
    assert np.array_equal(got["t"].view(np.uint32), ref_t.view(np.uint32))
    assert np.array_equal(got["instance"], ref_i) and np.array_equal(got["prim"], ref_p)


def test_tlas_normals_device_trace_and_hits(gpu, vx):
    import torch
    v, t = small_blob()
    b = vx.Bvh(vx.Mesh.from_arrays(v, t))
    inst = instance_ref.make_instances(random_transforms(32, seed=101))
    tl = vx.Tlas([b], inst)
    rays = np.concatenate([rays_around(3000, -9, 9, 102), grazing_axis_rays(1000, 103)])
    got = tl.trace_ex(rays, want=("t", "instance", "prim", "normal"))
    ref = instance_ref.world_normals([(v, t)], inst, got["instance"], got["prim"])
    assert np.allclose(got["normal"], ref, rtol=0, atol=4e-6), np.abs(got["normal"] - ref).max()
    assert np.allclose(np.linalg.norm(got["normal"][got["t"] > 0], axis=1), 1, atol=1e-6)
    n = len(rays)
    dr = torch.from_numpy(rays).cuda()
    dt, dp, di = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    db = torch.empty((n, 2), device="cuda")
    hits = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    nh = torch.zeros(1, dtype=torch.int64, device="cuda")
    tl.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr(), di.data_ptr(), db.data_ptr(), hits_ptr=hits.data_ptr(), nhits_ptr=nh.data_ptr())
    torch.cuda.synchronize()
    rt, ri, rp, rb = instance_ref.closest([(v, t)], inst, rays)
    assert np.array_equal(dt.cpu().numpy().view(np.uint32), rt.view(np.uint32))
    assert np.array_equal(di.cpu().numpy().view(np.uint32), ri) and np.array_equal(dp.cpu().numpy().view(np.uint32), rp)
    assert np.array_equal(db.cpu().numpy().view(np.uint32), rb.view(np.uint32))
    k = int(nh.item())
    assert k == int((rt > 0).sum())
    h = hits.cpu().numpy()[:k]
    order = np.argsort(h[:, 0])
    assert np.array_equal(h[order, 0], np.nonzero(rt > 0)[0])
    assert np.array_equal(h[order, 1].view(np.uint32), rp[rt > 0]) and np.array_equal(h[order, 2].view(np.float32), rt[rt > 0])


def test_tlas_and_blas_on_their_own_streams(gpu, vx):
    import torch
    bs, ts = torch.cuda.Stream(), torch.cuda.Stream()
    v, t = vx_scenes.scene("rotcube")
    mesh = vx.Mesh.from_arrays(v, t)
    b = vx.Bvh(mesh, stream=bs.cuda_stream)
    inst = instance_ref.make_instances(random_transforms(24, seed=111))
    tl = vx.Tlas([b], inst, stream=ts.cuda_stream)
    rays = rays_around(3000, -9, 9, 112)
    n = len(rays)
    dr = torch.from_numpy(rays).cuda()
    dt = torch.empty(n, device="cuda")
    dp = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tl.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr())   # queued on ts ...
    v2 = (v * np.float32(2.0)).astype(np.float32)
    b.build_into(vx.Mesh.from_arrays(v2, t))                          # ... a rebuild on bs must wait for it
    torch.cuda.synchronize()
    rt, _, rp, _ = instance_ref.closest([(v, t)], inst, rays)
    assert np.array_equal(dt.cpu().numpy().view(np.uint32), rt.view(np.uint32))
    tl.update(inst)                                                   # the update waits for bs (the rebuild) on ts
    check(tl, [(v2, t)], inst, rays, "after the rebuild on its own stream")


def test_cli_instances(gpu, vx, tmp_path):
    import subprocess
    import os
    pkg = os.path.dirname(vx.LIB_PATH)
    cv, ct = vx_scenes.scene("rotcube")
    obj = str(tmp_path / "c.obj")
    vx_scenes.write_obj(obj, cv, ct)
    tr = random_transforms(8, seed=121, spread=3.0)
    inf = tmp_path / "inst.txt"
    inf.write_text("\n".join(" ".join("%.9g" % x for x in row) for row in tr) + "\n")
    cli = os.path.join(pkg, "voxilizer")
    ok = subprocess.run([cli, obj, "0.1", "--render", str(tmp_path / "o.ppm"), "--size", "160x90", "--mesh", obj, "--instances", str(inf),
                         "--frames", "2"], capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0, ok.stderr
    assert "8 instances of the mesh" in ok.stdout and "device frame" in ok.stdout
    for extra in (["--render", str(tmp_path / "o.ppm"), "--mesh", obj], ["--render", str(tmp_path / "o.ppm"), "--frames", "2"], []):
        r = subprocess.run([cli, obj, "0.1"] + extra + ["--instances", str(inf)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--instances" in r.stderr, (extra, r.stderr)
