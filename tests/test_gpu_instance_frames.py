"""GPU tests of frames with instances (vx_render_create_tlas): a single identity instance gives the BVH scene's frame bit for bit, on the
grid and on the octree; non-identity scenes match render_ref fed from tests/instance_ref.py (kind and shadowed exact, rgba within 1 LSB);
triangle-only scenes; per-frame TLAS updates without allocation; stream ordering of a frame against a later update."""
import numpy as np
import pytest

import instance_ref
import oracle
import render_ref
import vx_scenes
from test_gpu_instances import random_transforms
from test_gpu_render import assert_lsb, write_two_material_cube
from test_gpu_render import reference as bvh_reference

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(0.05)


def camera(W, H, eye=(7.0, 5.0, -8.0), ctr=(0.0, 0.5, 0.0)):
    vi, pi = vx_scenes.camera_matrices(eye=eye, ctr=ctr, aspect=W / H)
    return vi, pi, W, H


def inst_shadow_rays(vi, d, kind, vt, mt, pos_tri, light=render_ref.DEFAULT_LIGHT):
    """render_ref.shadow_rays with the triangle hit point given (the instance's M * ((p0*b0 + p1*b1) + p2*b2))"""
    pos_l, _, ltype = light
    tri = kind == 2
    ts = np.where(tri, F(mt), np.where(F(vt) > 0, F(vt), F(0)))
    wp = F(vi[12:15])[None, :] + d * ts[:, None]
    if ltype == 1:
        l = np.broadcast_to(F(pos_l), wp.shape).astype(F)
    else:
        pos = wp.copy()
        pos[tri] = pos_tri[tri]
        l = F(pos_l)[None, :] - pos
    length = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2])
    L = l * (F(1) / length)[:, None]
    dist = np.full(length.shape, F(100000), F) if ltype == 1 else length
    return np.ascontiguousarray(np.concatenate([wp, L], 1).astype(F)), dist


def reference(vox, tl, meshes, mats, inst, cam, light=render_ref.DEFAULT_LIGHT):
    """render_ref over instance_ref's hits; meshes[b] = (verts, tris), mats[b] = (table, ids) or None"""
    vi, pi, W, H = cam
    n = W * H
    d = render_ref.host_dirs(vi, pi, W, H)
    prim_rays = oracle.primary_rays(vi, pi, W, H)   # the traversals' camera rays (load_ray), not render()'s shading directions
    if vox is not None:
        vo = vox.trace_ex(camera=cam, want=("t", "prim", "normal"))
    else:
        vo = {"t": np.full(n, -1, F), "normal": np.zeros((n, 3), F)}
    mt, mi, mp, mb = instance_ref.closest(meshes, inst, prim_rays)
    got = tl.trace_ex(camera=cam, want=("t", "instance", "prim", "normal"))   # the traversal agrees with the brute force ...
    assert np.array_equal(got["t"].view(np.uint32), mt.view(np.uint32)) and np.array_equal(got["instance"], mi)
    mn = got["normal"]                                                        # ... and the normal is the frame's own device function
    assert np.allclose(mn, instance_ref.world_normals(meshes, inst, mi, mp), atol=1e-5)
    kind = render_ref.merge(vo["t"], mt)
    pos = instance_ref.world_hit_points(meshes, inst, mi, mp, mb)
    rays, dist = inst_shadow_rays(vi, d, kind, vo["t"], mt, pos, light)
    sv = vox.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"] if vox is not None else np.zeros(n, np.uint8)
    sm = instance_ref.any_hit(meshes, inst, rays, tmax_per_ray=dist)
    mmat = None
    if any(m is not None for m in mats):
        mmat = render_ref.per_pixel_materials(None, np.full(n, -1), n)
        for b, m in enumerate(mats):
            if m is None:
                continue
            tab, ids = m
            sel = (mi != instance_ref.MISS)
            sel[sel] = inst["blas"][mi[sel]] == b
            pm = render_ref.per_pixel_materials(tab, np.where(sel, ids[np.minimum(mp, len(ids) - 1).astype(np.int64)], -1), n)
            for k in mmat:
                mmat[k][sel] = pm[k][sel]
    rgba, sh = render_ref.shade(d, kind, vo["normal"], mn, rays[:, 3:], dist, sv, sm, light, None, mmat)
    return dict(rgba=rgba, kind=kind, shadowed=sh, sm=sm.astype(bool))


def check(r, ref, cam, what):
    out = r.render_host(cam, want=("rgba", "kind", "shadowed"))
    n = cam[2] * cam[3]
    assert np.array_equal(out["kind"].ravel(), ref["kind"]), what + ": kind differs"
    assert np.array_equal(out["shadowed"].ravel(), ref["shadowed"]), what + ": shadowed differs"
    assert_lsb(out["rgba"].reshape(n, 4), ref["rgba"], what)
    return out


@pytest.mark.parametrize("source", ["grid", "octree"])
def test_identity_instance_frame_equals_bvh_frame(gpu, vx, source):
    v, t = vx_scenes.scene("atrium262k")
    mesh = vx.Mesh.from_arrays(v, t)
    vox = vx.Grid.voxelize(mesh, F(32.0 / 256)) if source == "grid" else vx.Octree(mesh, F(32.0 / 256))
    bvh = mesh.bvh()
    tl = vx.Tlas([bvh], vx.instances([instance_ref.transform()]))
    W, H = 640, 360
    for c in range(2):
        vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[c], aspect=W / H)
        cam = (vi, pi, W, H)
        a = vx.Renderer(vox, bvh, mesh).render_host(cam, want=("rgba", "kind", "shadowed"))
        b = vx.Renderer.from_tlas(vox, tl, [mesh]).render_host(cam, want=("rgba", "kind", "shadowed"))
        for k in ("rgba", "kind", "shadowed"):
            assert np.array_equal(a[k], b[k]), (source, c, k)
        assert (a["kind"] == 2).sum() + (a["kind"] == 1).sum() > 1000


def test_material_table_with_and_without_ids(gpu, vx):
    """Both scene forms gather a mesh's materials the same way: with a table but no per-triangle ids every triangle hit shades with
    MaterialObj{}, with ids by its triangle's record.  A two-triangle quad over a slab of voxels, 16 x 12: the BVH scene's frame is the
    identity-instance scene's bit for bit, and both are render_ref's picture (kind and shadowed exact, rgba within powf's 1 LSB)."""
    sv, st = vx_scenes.cube()
    vox = vx.Grid.voxelize(vx.Mesh.from_arrays(sv * F([0.4, 0.1, 0.4]), st), F(0.125))
    assert max(vox.describe()["dim"]) <= 8
    qv = F([[-0.2, 0.45, -0.2], [0.2, 0.45, -0.2], [0.2, 0.45, 0.2], [-0.2, 0.45, 0.2]])
    qt = np.int32([[0, 1, 2], [0, 2, 3]])
    mesh = vx.Mesh.from_arrays(qv, qt)
    bvh = mesh.bvh()
    tl = vx.Tlas([bvh], vx.instances([instance_ref.transform()]))
    mats = np.zeros(2, vx.MATERIAL)
    mats["ambient"] = F([[0.2, 0.05, 0.05], [0.02, 0.1, 0.1]])
    mats["diffuse"] = F([[0.8, 0.2, 0.1], [0.1, 0.6, 0.6]])
    mats["specular"] = F([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0]])
    mats["shininess"] = F([32, 1])
    mats["illum"] = [2, 1]
    W, H = 16, 12
    cam = camera(W, H, eye=(0.35, 0.9, -0.55), ctr=(0.0, 0.2, 0.0))
    hit = bvh.trace_ex(camera=cam, want=("t", "prim"))
    assert set(hit["prim"][hit["t"] > 0].tolist()) == {0, 1}           # the camera sees both triangles
    seen = {}
    for ids in (None, np.int32([1, 0])):
        what = "table only" if ids is None else "table and ids"
        mesh.set_materials(mats, ids)
        ref = bvh_reference(vox, W, H, cam[0], cam[1], bvh, (qv, qt, mats, ids))
        tri = ref["kind"] == 2
        assert tri.sum() >= 12 and (ref["kind"] == 1).sum() >= 30, what
        a = check(vx.Renderer(vox, bvh, mesh), ref, cam, what + ", BVH scene")
        b = check(vx.Renderer.from_tlas(vox, tl, [mesh]), ref, cam, what + ", identity instance")
        for k in ("rgba", "kind", "shadowed"):
            assert np.array_equal(a[k], b[k]), (what, k)
        seen[what] = a["rgba"].reshape(-1, 4)[tri]
    assert (np.abs(seen["table only"].astype(int) - seen["table and ids"].astype(int)).max(1) > 1).all()   # no pixel passes as the other case's


def instanced_scene(vx, tmp_path, n=16, seed=7):
    cv, ct = vx_scenes.rotated_cube(half=0.5)
    path = str(tmp_path / "two.obj")
    write_two_material_cube(path)
    model = vx.Mesh.load_obj(path)
    mv, mt_ = model.host_arrays()
    mats, ids = model.materials()
    fv = F([[-6, -1.5, -6], [6, -1.5, -6], [6, -1.5, 6], [-6, -1.5, 6]])
    ft = np.int32([[0, 1, 2], [0, 2, 3]])
    m0, m2 = vx.Mesh.from_arrays(cv, ct), vx.Mesh.from_arrays(fv, ft)
    meshes = [m0, model, m2]
    blas = [m.bvh() for m in meshes]
    tr = list(random_transforms(n, seed=seed, spread=3.0)) + [instance_ref.transform()]
    inst = instance_ref.make_instances(tr, blas=[k % 2 for k in range(n)] + [2])
    tl = vx.Tlas(blas, inst)
    return meshes, blas, tl, inst, [(cv, ct), (mv, mt_), (fv, ft)], [None, (mats, ids), None]


@pytest.mark.parametrize("voxels", [True, False])
def test_instanced_frame_vs_reference(gpu, vx, tmp_path, voxels):
    meshes, blas, tl, inst, host, mats = instanced_scene(vx, tmp_path)
    vox = None
    if voxels:
        bv, bt = vx_scenes.cube(half=0.75, center=(0.0, 3.5, 0.0))
        vox = vx.Grid.voxelize(vx.Mesh.from_arrays(bv, bt), VS)
    r = vx.Renderer.from_tlas(vox, tl, meshes)
    cam = camera(240, 135)
    ref = reference(vox, tl, host, mats, inst, cam)
    assert (ref["kind"] == 2).sum() > 1000 and ref["shadowed"].sum() > 50
    if voxels:
        assert (ref["kind"] == 1).sum() > 50
    check(r, ref, cam, "voxels" if voxels else "triangles only")
    lt = ((3.0, 10.0, -2.0), 1.0, 1)
    ref = reference(vox, tl, host, mats, inst, cam, lt)
    out = r.render_host(cam, lt, want=("rgba", "kind", "shadowed"))
    assert np.array_equal(out["kind"].ravel(), ref["kind"]) and np.array_equal(out["shadowed"].ravel(), ref["shadowed"])
    assert_lsb(out["rgba"].reshape(-1, 4), ref["rgba"], "directional")


def test_frames_with_updates_allocate_nothing(gpu, vx, tmp_path):
    import torch
    meshes, blas, tl, inst, host, mats = instanced_scene(vx, tmp_path)
    r = vx.Renderer.from_tlas(None, tl, meshes)
    cam = camera(320, 180)
    out = torch.empty((180, 320, 4), dtype=torch.uint8, device="cuda")
    recs = [instance_ref.make_instances(list(random_transforms(16, seed=100 + k, spread=3.0)) + [instance_ref.transform()],
                                        blas=list(inst["blas"])) for k in range(4)]
    devs = [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in recs]
    tl.update(recs[0])
    r.render(cam, out=out)
    torch.cuda.synchronize()
    a0 = vx.lib().vx_device_allocations()
    for k in range(4):
        tl.update(device_ptr=devs[k], count=len(recs[k]))
        r.render(cam, out=out)
        tl.update(recs[k])
        r.render(cam, out=out)
    torch.cuda.synchronize()
    assert vx.lib().vx_device_allocations() == a0
    ref = reference(None, tl, host, mats, recs[3], cam)
    assert_lsb(out.cpu().numpy().reshape(-1, 4), ref["rgba"], "after updates")


def test_frame_not_affected_by_a_later_update(gpu, vx, tmp_path):
    import torch
    meshes, blas, tl_unused, inst, host, mats = instanced_scene(vx, tmp_path)
    ts, fs = torch.cuda.Stream(), torch.cuda.Stream()
    tl = vx.Tlas(blas, inst, stream=ts)
    r = vx.Renderer.from_tlas(None, tl, meshes, stream=fs)
    cam = camera(320, 180)
    old = r.render_host(cam)["rgba"]
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += F(0.7)
    dev = torch.from_numpy(moved.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    out = torch.empty((180, 320, 4), dtype=torch.uint8, device="cuda")
    r.render(cam, out=out)                                # queued on fs ...
    tl.update(device_ptr=dev, count=len(moved))           # ... the update on ts, no host synchronisation in between
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), old)
    new = r.render_host(cam)["rgba"]
    assert not np.array_equal(new, old)
    ref = reference(None, tl, host, mats, moved, cam)
    assert_lsb(new.reshape(-1, 4), ref["rgba"], "after the update")


def test_render_create_tlas_errors(gpu, vx, tmp_path):
    meshes, blas, tl, inst, host, mats = instanced_scene(vx, tmp_path)
    with pytest.raises(vx.VxError):
        vx.Renderer.from_tlas(None, tl, meshes[:2])
    with pytest.raises(vx.VxError):
        vx.Renderer.from_tlas(None, tl, [meshes[2], meshes[1], meshes[0]])   # triangle counts differ from the BLAS's
    with pytest.raises(vx.VxError):
        vx.Renderer.from_tlas(None, None, meshes)
