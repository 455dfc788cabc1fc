"""GPU tests of attribute shading (vx_render_set_shading(VX_RENDER_ATTRIBUTES), Renderer(attributes=True)): kind and shadowed exact and rgba
within 1 LSB of tests/attr_ref.py over the Python API's traces, on smooth-normal, textured, normal-less and zero-normal meshes, point and
directional lights, BVH and TLAS scenes (identity instances bit-identical to the BVH scene); no allocation per frame, vx_render_refresh, the
switch back to the default shading, voxilizer --attributes, and a 4K frame of the blob field."""
import os
import subprocess

import numpy as np
import pytest

import attr_ref
import instance_ref
import render_ref
import vx_scenes
from test_gpu_instance_frames import inst_shadow_rays
from test_gpu_instances import random_transforms
from test_gpu_render import assert_lsb, read_ppm

pytestmark = pytest.mark.gpu

F = np.float32
DIRECTIONAL = ((3.0, 10.0, -2.0), 1.0, 1)


def camera(W, H, eye=(5.0, 6.0, -7.0), ctr=(0.0, 0.5, 0.0)):
    vi, pi = vx_scenes.camera_matrices(eye=eye, ctr=ctr, aspect=W / H)
    return vi, pi, W, H


def bvh_reference(vox, bvh, mesh, cam, light=render_ref.DEFAULT_LIGHT):
    vi, pi, W, H = cam
    vo = vox.trace_ex(camera=cam, want=("t", "prim", "normal"))
    mo = bvh.trace_ex(camera=cam, want=("t", "prim", "normal", "bary"))
    kind = render_ref.merge(vo["t"], mo["t"])
    d = render_ref.host_dirs(vi, pi, W, H)
    v, t = mesh.host_arrays()
    rays, dist = render_ref.shadow_rays(F(vi[12:15]), d, kind, vo["t"], mo["t"], mo["prim"], mo["bary"], v, t, light)
    sv = vox.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"]
    sm = bvh.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"]
    return attr_ref.frame(cam, vo, mo, [attr_ref.MeshAttr.of(mesh)], sv, sm, rays, dist, light)


def world_hit_points(host, inst, instance, prim, bary):
    """instance_ref.world_hit_points vectorised: M * ((p0*b0 + p1*b1) + p2*b2) per hit pixel, zeros elsewhere"""
    out = np.zeros((len(instance), 3), F)
    k = np.flatnonzero(instance != instance_ref.MISS)
    ii = instance[k].astype(np.int64)
    b0, b1, b2 = attr_ref.bary3(F(bary)[k])
    for b in np.unique(np.asarray(inst["blas"])[ii]):
        sel = np.asarray(inst["blas"])[ii] == b
        v, t = host[int(b)]
        p = F(v)[np.asarray(t)[prim[k[sel]].astype(np.int64)]]
        h = attr_ref.interp(p, b0[sel], b1[sel], b2[sel])
        m = F(inst["transform"])[ii[sel]]
        out[k[sel]] = np.stack([((m[:, 4 * r] * h[:, 0] + m[:, 4 * r + 1] * h[:, 1]) + m[:, 4 * r + 2] * h[:, 2]) + m[:, 4 * r + 3]
                                for r in range(3)], 1)
    return out


def tlas_reference(vox, tl, meshes, inst, cam, light=render_ref.DEFAULT_LIGHT):
    vi, pi, W, H = cam
    n = W * H
    vo = vox.trace_ex(camera=cam, want=("t", "prim", "normal")) if vox is not None else None
    mo = tl.trace_ex(camera=cam, want=("t", "instance", "prim", "bary", "normal"))
    vt = vo["t"] if vo is not None else np.full(n, -1, F)
    kind = render_ref.merge(vt, mo["t"])
    d = render_ref.host_dirs(vi, pi, W, H)
    host = [m.host_arrays() for m in meshes]
    pos = world_hit_points(host, inst, mo["instance"], mo["prim"], mo["bary"])
    rays, dist = inst_shadow_rays(vi, d, kind, vt, mo["t"], pos, light)
    sv = vox.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"] if vox is not None else np.zeros(n, np.uint8)
    sm = tl.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"]
    return attr_ref.frame(cam, vo, mo, [attr_ref.MeshAttr.of(m) for m in meshes], sv, sm, rays, dist, light, inst, tl.world_to_object())


def check(r, ref, cam, light=None, what=""):
    out = r.render_host(cam, light, want=("rgba", "kind", "shadowed"))
    n = cam[2] * cam[3]
    assert np.array_equal(out["kind"].ravel(), ref["kind"]), what + ": kind differs"
    assert np.array_equal(out["shadowed"].ravel(), ref["shadowed"]), what + ": shadowed differs"
    assert_lsb(out["rgba"].reshape(n, 4), ref["rgba"], what)
    return out


def cube_voxels(vx, center=(2.2, 0.6, 0.0), half=0.6, vs=F(0.05)):
    bv, bt = vx_scenes.cube(half=half, center=center)
    return vx.Grid.voxelize(vx.Mesh.from_arrays(bv, bt), vs)


def smooth_blob(vx, nlon=48, nlat=33, scale=1.2, offset=(0.0, 0.9, 0.0)):
    v, t = vx_scenes.blob(nlon=nlon, nlat=nlat)
    v = (v * F(scale) + F(offset)).astype(F)
    nrm, uv = vx_scenes.smooth_attributes(v, t)
    m = vx.Mesh.from_arrays(v, t)
    m.set_attributes(nrm, uv)
    return m


def floor_mesh(vx, half=5.0, y=-0.4):
    fv = F([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]])
    return vx.Mesh.from_arrays(fv, np.int32([[0, 2, 1], [0, 3, 2]]))


def merged(vx, parts):
    """one Mesh from (Mesh, ...) parts with corner normals / uvs where a part has them (zeros elsewhere: no normals -> (0,0,0) corners)"""
    vs, ts, ns, us, off = [], [], [], [], 0
    for m in parts:
        v, t = m.host_arrays()
        vs.append(v)
        ts.append(t + off)
        off += len(v)
        n, u = m.corner_normals(), m.corner_uvs()
        ns.append(n if n is not None else np.zeros((len(t), 3, 3), F))
        us.append(u if u is not None else np.zeros((len(t), 3, 2), F))
    out = vx.Mesh.from_arrays(np.concatenate(vs), np.concatenate(ts))
    out.set_attributes(np.concatenate(ns), np.concatenate(us))
    return out


# ---- BVH scenes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [None, DIRECTIONAL])
def test_smooth_blob_beside_voxels(gpu, vx, light):
    mesh = smooth_blob(vx)
    bvh = mesh.bvh()
    vox = cube_voxels(vx)
    cam = camera(320, 180)
    r = vx.Renderer(vox, bvh, mesh, attributes=True)
    lt = render_ref.DEFAULT_LIGHT if light is None else light
    ref = bvh_reference(vox, bvh, mesh, cam, lt)
    out = check(r, ref, cam, light, "smooth blob")
    tri = out["kind"].ravel() == 2
    assert tri.sum() > 500 and (out["kind"] == 1).sum() > 100
    default = vx.Renderer(vox, bvh, mesh).render_host(cam, light)["rgba"].reshape(-1, 4)
    differs = (default[tri] != out["rgba"].reshape(-1, 4)[tri]).any(1)
    assert differs.mean() > 0.5, differs.mean()                      # the mode is active on most triangle pixels
    vox_px = out["kind"].ravel() == 1
    assert np.array_equal(default[vox_px], out["rgba"].reshape(-1, 4)[vox_px])   # voxel hits are shaded as by default


def write_textured_plane(tmp_path):
    """a 6x5 grid of quads at y = 0 with uvs from -1.3 to 2.6 (beyond [0, 1] and negative); materials: a 37x19 checker (PPM), a 1x1 TGA, a
    missing file, one without a texture; the last row of quads has no material"""
    img = vx_scenes.checker_texture(37, 19, cells=5, seed=2)
    (tmp_path / "checker.ppm").write_bytes(b"P6\n37 19\n255\n" + img[..., :3].tobytes())
    one = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 32, 0x28]) + bytes([40, 160, 220, 255])   # BGRA (220, 160, 40)
    (tmp_path / "one.tga").write_bytes(one)
    (tmp_path / "plane.mtl").write_text("newmtl chk\nKa 0.1 0.1 0.1\nKd 0.9 0.8 0.7\nKs 0.4 0.4 0.4\nNs 16\nillum 2\nmap_Kd -bm 1 checker.ppm\n"
                                        "newmtl one\nKa 0.05 0.05 0.05\nKd 1 1 1\nillum 1\nmap_Kd one.tga\n"
                                        "newmtl gone\nKd 0.5 0.5 0.5\nillum 1\nmap_Kd nothere.ppm\n"
                                        "newmtl flat\nKd 0.3 0.6 0.3\nillum 1\n")
    nx, nz = 6, 5
    lines = ["mtllib plane.mtl"]
    for j in range(nz + 1):
        for i in range(nx + 1):
            lines.append("v %g 0 %g" % (-3.0 + i, -2.0 + j))
            lines.append("vt %g %g" % (-1.3 + 3.9 * i / nx, 2.6 - 3.9 * j / nz))
    lines.append("vn 0 1 0")
    mats = ["chk", "one", "gone", "flat", "nosuch"]
    for j in range(nz):
        lines.append("usemtl %s" % mats[j])
        for i in range(nx):
            a = j * (nx + 1) + i + 1
            b, c, d = a + 1, a + nx + 2, a + nx + 1
            vn = "1" if (i + j) % 2 == 0 else ""                             # half the quads smooth (+y), half without a vn (zero normal)
            lines.append("f %d/%d/%s %d/%d/%s %d/%d/%s %d/%d/%s" % (a, a, vn, d, d, vn, c, c, vn, b, b, vn))
    (tmp_path / "plane.obj").write_text("\n".join(lines) + "\n")
    return tmp_path / "plane.obj", img


@pytest.mark.parametrize("light", [None, DIRECTIONAL])
def test_textured_plane(gpu, vx, tmp_path, light):
    obj, img = write_textured_plane(tmp_path)
    mesh = vx.Mesh.load_obj(str(obj))
    assert mesh.material_textures().tolist() == [0, 1, 2, -1]
    mesh.load_textures()
    assert np.array_equal(mesh.texture(0), img) and mesh.texture(1).tolist() == [[[220, 160, 40, 255]]]
    assert mesh.texture(2).tolist() == [[[255, 0, 255, 255]]]
    bvh = mesh.bvh()
    vox = cube_voxels(vx, center=(0.0, 1.5, 0.0), half=0.4)
    cam = camera(320, 200, eye=(0.5, 5.0, -4.0), ctr=(0.0, 0.0, 0.0))
    r = vx.Renderer(vox, bvh, mesh, attributes=True)
    lt = render_ref.DEFAULT_LIGHT if light is None else light
    ref = bvh_reference(vox, bvh, mesh, cam, lt)
    out = check(r, ref, cam, light, "textured plane")
    assert (out["kind"] == 2).sum() > 10000
    rgb = out["rgba"].reshape(-1, 4)[:, :3]
    magenta = (rgb[:, 1] == 0) & (rgb[:, 0] > 30) & (np.abs(rgb[:, 0].astype(int) - rgb[:, 2]) <= 1)
    assert magenta.sum() > 500                                                           # the missing file is magenta


def test_back_faces_without_vn_are_unlit(gpu, vx):
    # a floor wound downward (face normal -y) seen from above, the light above: lit by default (turned toward the ray), unlit here
    fv = F([[-4, 0, -4], [4, 0, -4], [4, 0, 4], [-4, 0, 4]])
    mesh = vx.Mesh.from_arrays(fv, np.int32([[0, 1, 2], [0, 2, 3]]))
    bvh = mesh.bvh()
    vox = cube_voxels(vx, center=(0.0, 1.0, 0.0), half=0.5)
    cam = camera(240, 160, eye=(1.0, 6.0, -5.0), ctr=(0.0, 0.0, 0.0))
    r = vx.Renderer(vox, bvh, mesh, attributes=True)
    ref = bvh_reference(vox, bvh, mesh, cam)
    out = check(r, ref, cam, None, "back faces")
    d = vx.Renderer(vox, bvh, mesh).render_host(cam, want=("rgba", "shadowed"))
    tri = out["kind"].ravel() == 2
    assert tri.sum() > 5000 and out["shadowed"].ravel()[tri].sum() == 0          # unlit: no shadow flag is read
    assert d["shadowed"].ravel()[tri].sum() > 100                               # the cube's shadow on the lit default floor
    assert (out["rgba"].reshape(-1, 4)[tri, :3].astype(int).sum(1) < d["rgba"].reshape(-1, 4)[tri, :3].astype(int).sum(1)).mean() > 0.9


def test_zero_normals_fall_back_to_default(gpu, vx):
    mesh = floor_mesh(vx)
    mesh.set_attributes(np.zeros((2, 3, 3), F))
    bvh = mesh.bvh()
    vox = cube_voxels(vx, center=(0.0, 0.8, 0.0), half=0.5)
    cam = camera(200, 120)
    r = vx.Renderer(vox, bvh, mesh, attributes=True)
    out = check(r, bvh_reference(vox, bvh, mesh, cam), cam, None, "zero normals")
    d = vx.Renderer(vox, bvh, mesh).render_host(cam, want=("rgba", "kind", "shadowed"))
    assert (out["kind"] == 2).sum() > 3000
    for k in ("rgba", "kind", "shadowed"):
        assert np.array_equal(out[k], d[k]), k


def test_switch_refresh_and_no_allocation(gpu, vx, tmp_path):
    import torch
    obj, img = write_textured_plane(tmp_path)
    mesh = vx.Mesh.load_obj(str(obj))
    mesh.load_textures()
    bvh = mesh.bvh()
    vox = cube_voxels(vx, center=(0.0, 1.5, 0.0), half=0.4)
    cam = camera(256, 160, eye=(0.5, 5.0, -4.0), ctr=(0.0, 0.0, 0.0))
    default = vx.Renderer(vox, bvh, mesh).render_host(cam, want=("rgba", "kind", "shadowed"))
    r = vx.Renderer(vox, bvh, mesh, attributes=True)
    out = torch.empty((160, 256, 4), dtype=torch.uint8, device="cuda")
    r.render(cam, out=out)
    torch.cuda.synchronize()
    a0 = vx.lib().vx_device_allocations()
    for _ in range(4):
        r.render(cam, out=out)
    torch.cuda.synchronize()
    assert vx.lib().vx_device_allocations() == a0
    assert_lsb(out.cpu().numpy().reshape(-1, 4), bvh_reference(vox, bvh, mesh, cam)["rgba"], "steady state")
    r.set_shading(0)
    back = r.render_host(cam, want=("rgba", "kind", "shadowed"))
    for k in back:
        assert np.array_equal(back[k], default[k]), k                       # mode 0: the default frame bit for bit
    with pytest.raises(vx.VxError):
        r.set_shading(2)
    r.set_shading(vx.RENDER_ATTRIBUTES)
    before = r.render_host(cam)["rgba"]
    mesh.set_texture(0, 255 - img)                                          # picked up by refresh only
    n = mesh.corner_normals()
    n[:] = F([0.0, 1.0, 0.2])
    mesh.set_attributes(n, mesh.corner_uvs())
    assert np.array_equal(r.render_host(cam)["rgba"], before)
    r.refresh()
    after = r.render_host(cam, want=("rgba", "kind", "shadowed"))
    assert not np.array_equal(after["rgba"], before)
    ref = bvh_reference(vox, bvh, mesh, cam)
    assert np.array_equal(after["kind"].ravel(), ref["kind"]) and np.array_equal(after["shadowed"].ravel(), ref["shadowed"])
    assert_lsb(after["rgba"].reshape(-1, 4), ref["rgba"], "after refresh")


# ---- instanced scenes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["grid", "octree"])
def test_identity_instance_equals_bvh_scene(gpu, vx, tmp_path, source):
    obj, _ = write_textured_plane(tmp_path)
    plane = vx.Mesh.load_obj(str(obj))
    plane.load_textures()
    blob = smooth_blob(vx, offset=(0.0, 1.2, 0.0))
    mesh = merged(vx, [blob])
    bv, bt = vx_scenes.cube(half=0.5, center=(2.0, 0.6, 0.5))
    vm = vx.Mesh.from_arrays(bv, bt)
    vox = vx.Grid.voxelize(vm, F(0.05)) if source == "grid" else vx.Octree(vm, F(0.05))
    cam = camera(256, 160, eye=(0.5, 5.0, -5.0), ctr=(0.0, 0.5, 0.0))
    for m in (mesh, plane):
        bvh = m.bvh()
        tl = vx.Tlas([bvh], vx.instances([instance_ref.transform()]))
        a = vx.Renderer(vox, bvh, m, attributes=True).render_host(cam, want=("rgba", "kind", "shadowed"))
        b = vx.Renderer.from_tlas(vox, tl, [m], attributes=True).render_host(cam, want=("rgba", "kind", "shadowed"))
        for k in a:
            assert np.array_equal(a[k], b[k]), (source, k)
        assert (a["kind"] == 2).sum() > 1000


def instanced(vx, tmp_path):
    obj, _ = write_textured_plane(tmp_path)
    plane = vx.Mesh.load_obj(str(obj))
    plane.load_textures()
    blob = smooth_blob(vx, nlon=32, nlat=21, scale=0.5, offset=(0.0, 0.0, 0.0))
    meshes = [blob, plane]
    blas = [m.bvh() for m in meshes]
    rng = np.random.default_rng(5)
    tr = list(random_transforms(12, seed=17, spread=2.5))                    # rotated, scaled, sheared, mirrored
    mirror = instance_ref.transform(rot=instance_ref.random_rotation(rng), scale=(-0.8, 0.6, 0.7), shear=0.4, offset=(1.5, 0.5, -1.0))
    floor = instance_ref.transform(rot=np.diag([1.0, -1.0, -1.0]), scale=(1.2, 1.0, 1.2), offset=(0.0, -1.5, 0.0))   # upside-down plane
    tr += [mirror, floor]
    inst = instance_ref.make_instances(tr, blas=[0] * 12 + [0, 1])
    return meshes, blas, vx.Tlas(blas, inst), inst


@pytest.mark.parametrize("voxels,light", [(True, None), (True, DIRECTIONAL), (False, None)])
def test_instanced_attribute_frames(gpu, vx, tmp_path, voxels, light):
    meshes, blas, tl, inst = instanced(vx, tmp_path)
    vox = cube_voxels(vx, center=(0.0, 3.0, 0.0), half=0.6) if voxels else None
    cam = camera(288, 162, eye=(6.0, 5.0, -7.0), ctr=(0.0, 0.0, 0.0))
    lt = render_ref.DEFAULT_LIGHT if light is None else light
    ref = tlas_reference(vox, tl, meshes, inst, cam, lt)
    assert (ref["kind"] == 2).sum() > 4000
    r = vx.Renderer.from_tlas(vox, tl, meshes, attributes=True)
    check(r, ref, cam, light, "instanced voxels=%s" % voxels)


def test_cli_attributes(gpu, vx, tmp_path):
    obj, _ = write_textured_plane(tmp_path)
    cube = tmp_path / "cube.obj"
    bv, bt = vx_scenes.cube(half=0.5, center=(0.0, 1.2, 0.0))
    vx_scenes.write_obj(str(cube), bv, bt)
    cli = os.path.join(os.path.dirname(vx.LIB_PATH), "voxilizer")
    W, H = 200, 120
    base = [cli, str(cube), "0.05", "--size", "%dx%d" % (W, H), "--mesh", str(obj)]
    out = tmp_path / "a.ppm"
    r = subprocess.run(base + ["--render", str(out), "--frames", "2", "--attributes", "--camera-dump", str(tmp_path / "cam.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cm = np.fromfile(tmp_path / "cam.bin", np.float32)
    cam = (cm[:16], cm[16:], W, H)
    mesh = vx.Mesh.load_obj(str(obj))
    mesh.load_textures()
    bvh = mesh.bvh()
    vox = vx.Grid.voxelize(vx.Mesh.load_obj(str(cube)), F(0.05))
    want = vx.Renderer(vox, bvh, mesh, attributes=True).render_host(cam)["rgba"].reshape(-1, 4)[:, :3]
    assert np.array_equal(read_ppm(str(out), W, H), want)
    r = subprocess.run(base + ["--render", str(out), "--attributes"], capture_output=True, text=True, timeout=120)    # no --frames
    assert r.returncode == 2 and "--attributes" in r.stderr, r.stderr
    r = subprocess.run([cli, str(cube), "0.05", "--render", str(out), "--frames", "2", "--attributes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--attributes" in r.stderr


def test_4k_blob_field(gpu, vx):
    f = vx_scenes.attr_blob_field()
    mesh = vx.Mesh.from_arrays(f["verts"], f["tris"])
    mesh.set_attributes(f["normals"], f["uvs"])
    rec = np.zeros(1, vx.MATERIAL)
    rec["ambient"], rec["diffuse"], rec["specular"], rec["shininess"], rec["illum"] = 0.05, 0.9, 0.3, 32.0, 2
    mesh.set_materials(rec, np.zeros(mesh.num_triangles, np.int32))
    mesh.set_material_textures([0])
    mesh.set_texture(0, f["texture"])
    inst = vx.instances(f["transforms"])
    tl = vx.Tlas([mesh.bvh()], inst)
    v, t = vx_scenes.scene("atrium262k")
    vox = vx.Grid.voxelize(vx.Mesh.from_arrays(v, t), F(32.0 / 256))
    meshes = [mesh]
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=3840 / 2160)
    cam = (vi, pi, 3840, 2160)
    ref = tlas_reference(vox, tl, meshes, inst, cam)
    assert (ref["kind"] == 2).sum() > 400000
    check(vx.Renderer.from_tlas(vox, tl, meshes, attributes=True), ref, cam, None, "4K blob field")
