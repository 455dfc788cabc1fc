"""GPU tests of device frames (vx_render_*, Renderer, voxilizer --frames): the picture of voxilizer --render within 1 LSB per channel, kind
and shadow masks identical to the numpy restatement over the Python API's ray queries (tests/render_ref.py), lights, steady state, stream
ordering against a rebuild, a 4K frame of the atrium and the edge cases."""
import os
import re

import numpy as np
import pytest

import render_ref
import vx_scenes
from test_gpu_mesh_trace import restate_mesh_render, run_cli, write_mesh_obj

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(0.05)


def cube_scene(tmp_path, with_mtl):
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    obj, mobj = tmp_path / "c.obj", tmp_path / "scene.obj"
    vx_scenes.write_obj(str(obj), v, t)
    write_mesh_obj(str(mobj), with_mtl)
    return v, t, obj, mobj


def write_two_material_cube(path):
    """the rotated cube with two usemtl groups (half of the triangles each) and their .mtl"""
    v, t = vx_scenes.rotated_cube(half=1.0, offset=(0.0, 1.0, 0.0))
    with open(os.path.join(os.path.dirname(path), "cube.mtl"), "w") as fh:
        fh.write("newmtl red\nKa 0.2 0.05 0.05\nKd 0.8 0.2 0.1\nKs 0.5 0.5 0.5\nNs 32\nillum 2\n")
        fh.write("newmtl teal\nKa 0.02 0.1 0.1\nKd 0.1 0.6 0.6\nKs 0 0 0\nNs 1\nillum 1\n")
    h = len(t) // 2
    lines = ["mtllib cube.mtl"] + ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    lines += ["usemtl red"] + ["f %d %d %d" % tuple(x) for x in (t[:h] + 1).tolist()]
    lines += ["usemtl teal"] + ["f %d %d %d" % tuple(x) for x in (t[h:] + 1).tolist()]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_ppm(path, W, H):
    raw = open(path, "rb").read()
    return np.frombuffer(raw[len(b"P6\n%d %d\n255\n" % (W, H)):], np.uint8).reshape(H * W, 3)


def hit_line(out):
    m = re.search(r"\[voxhip\] rendered \d+x\d+ to \S+: (.*)", out)
    assert m, out
    return m.group(1)


def reference(vox, W, H, vi, pi, bvh=None, model=None, light=render_ref.DEFAULT_LIGHT, vox_materials=None):
    """render_ref fed from the Python API's traces -> dict(rgba [n, 4], kind, shadowed, sv, sm); model = (verts, tris, mats, ids)"""
    cam = (vi, pi, W, H)
    vo = vox.trace_ex(camera=cam, want=("t", "prim", "normal"))
    mo = bvh.trace_ex(camera=cam, want=("t", "prim", "normal", "bary")) if bvh is not None else None
    kind = render_ref.merge(vo["t"], mo["t"] if mo else None)
    d = render_ref.host_dirs(vi, pi, W, H)
    if mo:
        mv, mt_, mats, ids = model
        rays, dist = render_ref.shadow_rays(F(vi[12:15]), d, kind, vo["t"], mo["t"], mo["prim"], mo["bary"], mv, mt_, light)
    else:
        rays, dist = render_ref.shadow_rays(F(vi[12:15]), d, kind, vo["t"], light=light)
    sv = vox.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"]
    sm = bvh.trace_ex(rays, tmax_per_ray=dist, any_hit=True, want=("shadowed",))["shadowed"] if mo else np.zeros_like(sv)
    n = W * H
    vmat = None
    if vox_materials is not None:
        tab, vids = vox_materials
        prim = vo["prim"].astype(np.int64)
        ok = (vo["t"] > 0) & (prim < len(vids))
        pid = np.full(n, -1, np.int64)
        pid[ok] = vids[prim[ok]]
        vmat = render_ref.per_pixel_materials(tab, pid, n)
    mmat = None
    if mo and model[3] is not None:
        mmat = render_ref.per_pixel_materials(model[2], model[3][np.minimum(mo["prim"], len(model[1]) - 1).astype(np.int64)], n)
    rgba, sh = render_ref.shade(d, kind, vo["normal"], mo["normal"] if mo else None, rays[:, 3:], dist, sv, sm, light, vmat, mmat)
    return dict(rgba=rgba, kind=kind, shadowed=sh, sv=sv.astype(bool), sm=sm.astype(bool))


def assert_lsb(img, ref, what):
    diff = np.abs(img.astype(np.int16) - ref.astype(np.int16)).max(axis=-1).ravel()
    bad = np.flatnonzero(diff > 1)
    assert bad.size == 0, "%s: %d pixels differ by more than 1 LSB, first %s: %s vs %s" % (what, bad.size, bad[:3], img.reshape(-1, img.shape[-1])[bad[:3]],
                                                                                         ref.reshape(-1, ref.shape[-1])[bad[:3]])


def check_frame(r, ref, cam, light=None, what=""):
    out = r.render_host(cam, light, want=("rgba", "kind", "shadowed"))
    n = cam[2] * cam[3]
    assert np.array_equal(out["kind"].ravel(), ref["kind"]), what + ": kind differs"
    assert np.array_equal(out["shadowed"].ravel(), ref["shadowed"]), what + ": shadowed differs"
    assert (out["rgba"].reshape(n, 4)[:, 3] == 255).all()
    assert_lsb(out["rgba"].reshape(n, 4), ref["rgba"], what)
    return out


def cam_dump(tmp_path, obj, W, H):
    cam = tmp_path / "cam.bin"
    r = run_cli([str(obj), "0.05", "--render", str(tmp_path / "cam.ppm"), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)])
    assert r.returncode == 0, r.stdout
    cm = np.fromfile(cam, np.float32)
    return cm[:16], cm[16:]


# ---- 0. the restatement against the one of test_gpu_mesh_trace ----------------------------------------------------------------------
@pytest.mark.parametrize("grid,with_mtl", [("bool", True), ("octree", False)])
def test_render_ref_matches_mesh_restatement(gpu, tmp_path, grid, with_mtl):
    v, t, obj, mobj = cube_scene(tmp_path, with_mtl)
    W, H = 320, 180
    vi, pi = cam_dump(tmp_path, obj, W, H)
    mesh = gpu.Mesh.from_arrays(v, t)
    vox = gpu.Grid.voxelize(mesh, VS) if grid == "bool" else gpu.Octree(mesh, VS)
    model = gpu.Mesh.load_obj(str(mobj))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    bvh = model.bvh()
    img, tri, sv, sm = restate_mesh_render(vox, bvh, mv, mtris, mats, ids, vi, pi, W, H)
    ref = reference(vox, W, H, vi, pi, bvh, (mv, mtris, mats, ids))
    assert np.array_equal(ref["rgba"][:, :3], img)
    assert np.array_equal(ref["kind"] == 2, tri) and np.array_equal(ref["sv"], sv) and np.array_equal(ref["sm"], sm)


# ---- 1. against the CLI, with and without --frames ---------------------------------------------------------------------------------
VARIANTS = [("bool", "mesh_mtl"), ("octree", "mesh"), ("bool", "materials"), ("octree", "plain")]


@pytest.mark.parametrize("grid,variant", VARIANTS)
def test_cli_frames_match_host_render(gpu, tmp_path, grid, variant):
    W, H = 320, 180
    v, t, obj, mobj = cube_scene(tmp_path, variant == "mesh_mtl")
    extra = ["--mesh", str(mobj)] if variant.startswith("mesh") else []
    if variant == "materials":
        obj = tmp_path / "cube2.obj"
        write_two_material_cube(str(obj))
        extra = ["--materials"]
    args = [str(obj), "0.05", "--grid", grid, "--size", "%dx%d" % (W, H)] + extra
    a, b = tmp_path / "host.ppm", tmp_path / "dev.ppm"
    r0 = run_cli(args + ["--render", str(a)])
    r1 = run_cli(args + ["--render", str(b), "--frames", "3"])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout + r1.stdout
    assert hit_line(r0.stdout) == hit_line(r1.stdout)
    assert re.search(r"\[voxhip\] device frame %dx%d: [0-9.]+ ms/frame \([0-9.]+ FPS\) over 2 frames" % (W, H), r1.stdout), r1.stdout
    ia, ib = read_ppm(a, W, H), read_ppm(b, W, H)
    assert_lsb(ib, ia, "--frames vs --render")
    assert len(np.unique(ia, axis=0)) > 8


def test_cli_frames_refusals(gpu, tmp_path):
    v, t, obj, mobj = cube_scene(tmp_path, False)
    for extra in (["--frames", "2"], ["--render", str(tmp_path / "x.ppm"), "--frames", "2", "--bench", "2"],
                  ["--render", str(tmp_path / "x.ppm"), "--frames", "2", "--grid", "vec"]):
        r = run_cli([str(obj), "0.05"] + extra)
        assert r.returncode != 0 and "--frames renders with --render" in r.stdout, extra


# ---- 2. exact classification through Renderer.render_host ------------------------------------------------------------------------
@pytest.mark.parametrize("grid,with_mtl", [("bool", True), ("octree", False)])
def test_render_host_classification(gpu, tmp_path, grid, with_mtl):
    v, t, obj, mobj = cube_scene(tmp_path, with_mtl)
    W, H = 320, 180
    vi, pi = cam_dump(tmp_path, obj, W, H)
    mesh = gpu.Mesh.from_arrays(v, t)
    vox = gpu.Grid.voxelize(mesh, VS) if grid == "bool" else gpu.Octree(mesh, VS)
    model = gpu.Mesh.load_obj(str(mobj))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    bvh = model.bvh()
    ref = reference(vox, W, H, vi, pi, bvh, (mv, mtris, mats, ids))
    tri = ref["kind"] == 2
    floor_shadow = tri & ref["sv"]
    vox_by_mesh = (ref["kind"] == 1) & ref["sm"] & ~ref["sv"]
    assert floor_shadow.sum() >= 20 and vox_by_mesh.sum() >= 20, (floor_shadow.sum(), vox_by_mesh.sum())
    r = gpu.Renderer(vox, bvh, model)
    check_frame(r, ref, (vi, pi, W, H), what=grid)
    r.free()


# ---- 3. lights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [((3.0, 10.0, 2.0), 1.2, 1), ((-6.0, 30.0, 4.0), 700.0, 0)], ids=["directional", "moved_point"])
def test_render_lights(gpu, tmp_path, light):
    v, t, obj, mobj = cube_scene(tmp_path, True)
    W, H = 320, 180
    vi, pi = cam_dump(tmp_path, obj, W, H)
    mesh = gpu.Mesh.from_arrays(v, t)
    vox = gpu.Grid.voxelize(mesh, VS)
    model = gpu.Mesh.load_obj(str(mobj))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    bvh = model.bvh()
    lt = (F(light[0]), F(light[1]), light[2])
    ref = reference(vox, W, H, vi, pi, bvh, (mv, mtris, mats, ids), light=lt)
    assert ref["shadowed"].sum() >= 20 and (ref["kind"] == 2).sum() >= 200
    r = gpu.Renderer(vox, bvh, model)
    check_frame(r, ref, (vi, pi, W, H), light, what=str(light))
    base = r.render_host((vi, pi, W, H))["rgba"]
    assert not np.array_equal(base, r.render_host((vi, pi, W, H), light)["rgba"])


# ---- 4. steady state: no allocation, identical frames, rebuilds ----------------------------------------------------------------------
def test_render_steady_state_and_rebuilds(gpu, tmp_path):
    import torch
    v, t, obj, mobj = cube_scene(tmp_path, True)
    W, H = 320, 180
    vi, pi = cam_dump(tmp_path, obj, W, H)
    cam = (vi, pi, W, H)
    mesh = gpu.Mesh.from_arrays(v, t)
    grid = gpu.Grid.voxelize(mesh, VS)
    model = gpu.Mesh.load_obj(str(mobj))
    bvh = model.bvh()
    r = gpu.Renderer(grid, bvh, model)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    r.render(cam, out=out)
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    n0 = gpu.device_allocations()
    for _ in range(19):
        r.render(cam, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), first)
    assert gpu.device_allocations() == n0, "a frame of a size already rendered requested device memory"
    # a rebuild at another voxel size, then refresh(): the next frame is the CLI's at that size
    grid.revoxelize(mesh, F(0.07))
    r.refresh()
    ppm = tmp_path / "vs07.ppm"
    rc = run_cli([str(obj), "0.07", "--size", "%dx%d" % (W, H), "--render", str(ppm), "--mesh", str(mobj)])
    assert rc.returncode == 0, rc.stdout
    img = r.render(cam, out=out)
    torch.cuda.synchronize()
    assert_lsb(img.cpu().numpy().reshape(-1, 4)[:, :3], read_ppm(ppm, W, H), "after revoxelize + refresh")
    assert not np.array_equal(img.cpu().numpy(), first)


def test_render_picks_up_bvh_build_into(gpu, tmp_path):
    import torch
    v, t, obj, _ = cube_scene(tmp_path, False)
    W, H = 320, 180
    vi, pi = cam_dump(tmp_path, obj, W, H)
    cam = (vi, pi, W, H)
    grid = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), VS)
    fv = torch.tensor([[-6, -0.8, -6], [6, -0.8, -6], [6, -0.8, 6], [-6, -0.8, 6]], dtype=torch.float32, device="cuda")
    ft = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device="cuda")
    model = gpu.Mesh.from_device(fv.data_ptr(), 4, ft.data_ptr(), 2, keep=(fv, ft))
    bvh = model.bvh()
    r = gpu.Renderer(grid, bvh, model)
    before = r.render_host(cam, want=("rgba", "kind"))
    fv[:, 1] = -0.3                                    # the floor moves up into the cube
    torch.cuda.synchronize()
    bvh.build_into(model)
    after = r.render_host(cam, want=("rgba", "kind", "shadowed"))
    ref = reference(grid, W, H, vi, pi, bvh, (fv.cpu().numpy(), ft.cpu().numpy(), None, None))
    assert np.array_equal(after["kind"].ravel(), ref["kind"]) and np.array_equal(after["shadowed"].ravel(), ref["shadowed"])
    assert_lsb(after["rgba"].reshape(-1, 4), ref["rgba"], "after build_into")
    assert not np.array_equal(before["kind"], after["kind"])


# ---- 5. stream ordering: a rebuild on the grid's stream queued behind a frame on the scene's stream --------------------------------------
def test_render_stream_ordering(gpu, tmp_path):
    import torch
    v, t, obj, mobj = cube_scene(tmp_path, False)
    W, H = 640, 360
    vi, pi = cam_dump(tmp_path, obj, W, H)
    cam = (vi, pi, W, H)
    gs, fs = torch.cuda.Stream(), torch.cuda.Stream()
    mesh = gpu.Mesh.from_arrays(v, t)
    grid = gpu.Grid.voxelize(mesh, VS, stream=gs.cuda_stream)
    model = gpu.Mesh.load_obj(str(mobj))
    bvh = model.bvh()
    r = gpu.Renderer(grid, bvh, model, stream=fs)
    old = r.render_host(cam)["rgba"]                   # the old grid, after a synchronise
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    r.render(cam, out=out)                             # queued on fs ...
    grid.revoxelize(mesh, F(0.11), stream=gs.cuda_stream)   # ... and the rebuild on gs, no host synchronisation in between
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), old)
    assert not np.array_equal(r.render_host(cam)["rgba"], old)


# ---- 6. size: the atrium at 512^3 with its mesh, 3840x2160 from the interior camera ---------------------------------------------------
def test_render_atrium_4k(gpu):
    v, t = vx_scenes.scene("atrium262k")
    mesh = gpu.Mesh.from_arrays(v, t)
    grid = gpu.Grid.voxelize(mesh, F(32.0 / 512))
    bvh = mesh.bvh()
    W, H = 3840, 2160
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=W / H)
    ref = reference(grid, W, H, vi, pi, bvh, (v, t, None, None))
    # the voxels are a conservative cover of the same triangles, so a voxel is met first (or at equal t) on every primary ray: the mesh
    # takes part through its traversal and its shadow rays
    assert (ref["kind"] == 1).sum() > 1000 and ref["shadowed"].sum() > 1000 and ref["sm"].sum() > 1000
    r = gpu.Renderer(grid, bvh, mesh)
    check_frame(r, ref, (vi, pi, W, H), what="atrium 4K")


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------
def test_render_edges(gpu, tmp_path):
    v, t, obj, mobj = cube_scene(tmp_path, True)
    mesh = gpu.Mesh.from_arrays(v, t)
    grid = gpu.Grid.voxelize(mesh, VS)
    model = gpu.Mesh.load_obj(str(mobj))
    mv, mtris = model.host_arrays()
    mats, ids = model.materials()
    bvh = model.bvh()
    r = gpu.Renderer(grid, bvh, model)
    for W, H in ((1, 1), (333, 7), (257, 3)):
        vi, pi = vx_scenes.camera_matrices(aspect=W / H)
        check_frame(r, reference(grid, W, H, vi, pi, bvh, (mv, mtris, mats, ids)), (vi, pi, W, H), what="%dx%d" % (W, H))
    # a camera facing away: every pixel is the miss colour
    vi, pi = vx_scenes.camera_matrices(eye=(6.0, 2.0, -3.0), ctr=(12.0, 3.0, -6.0), aspect=2.0)
    out = r.render_host((vi, pi, 64, 32), want=("rgba", "kind", "shadowed"))
    assert (out["kind"] == 0).all() and (out["shadowed"] == 0).all() and (out["rgba"].reshape(-1, 4) == [230, 230, 230, 255]).all()
    W, H = 160, 90
    vi, pi = vx_scenes.camera_matrices(aspect=W / H)
    # a mesh without triangles
    empty = gpu.Mesh.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    eb = empty.bvh()
    re_ = gpu.Renderer(grid, eb, empty)
    ref = reference(grid, W, H, vi, pi, eb, (np.zeros((0, 3), F), np.zeros((0, 3), np.int32), None, None))
    assert (ref["kind"] == 1).sum() > 100 and not (ref["kind"] == 2).any()
    check_frame(re_, ref, (vi, pi, W, H), what="empty mesh")
    # no mesh at all: the same picture
    rn = gpu.Renderer(grid)
    check_frame(rn, ref, (vi, pi, W, H), what="no mesh")
    # a grid without an occupied voxel: the mesh alone
    g0 = gpu.Grid.create(gpu.GRID_BOOL, 16, 16, 16, 0.1, origin=(-0.8, 0.0, -0.8))
    r0 = gpu.Renderer(g0, bvh, model)
    ref = reference(g0, W, H, vi, pi, bvh, (mv, mtris, mats, ids))
    assert not (ref["kind"] == 1).any() and (ref["kind"] == 2).sum() > 100
    check_frame(r0, ref, (vi, pi, W, H), what="empty grid")
    # argument errors that need real handles
    with pytest.raises(gpu.VxError) as e:
        gpu.Renderer(gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC))
    assert e.value.status == 1 and "VX_GRID_BOOL" in e.value.message
    with pytest.raises(gpu.VxError) as e:
        gpu.Renderer(grid, bvh, mesh)
    assert e.value.status == 1 and "triangle count" in e.value.message
    for x in (r, re_, rn, r0):
        x.free()
