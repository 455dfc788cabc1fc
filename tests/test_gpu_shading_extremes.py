"""GPU tests of the eight frame shaders (k_render_shadow_rays[_tlas|_attr|_attr_tlas], k_render_shade[_tlas|_attr|_attr_tlas]) at material,
light, normal and texture extremes (tests/shading_extremes.py; include/voxhip.h "shading at its extremes").  Every frame
is compared with the high-precision evaluation over the GPU's own traversal outputs: kind and shadowed exact, every channel of a hit pixel
EXACT unless 255 * c^(1/2.2) lies within shading_extremes.M_TIE of a rounding tie.  Every case runs as a BVH scene and as a TLAS scene with
one identity instance, which must equal the BVH frame bit for bit."""
import functools

import numpy as np
import pytest

import instance_ref
import shading_extremes as sx
import vx_scenes

pytestmark = pytest.mark.gpu

F = np.float32
MODES = [False, True]
MODE_IDS = ["default", "attributes"]
WANT = ("rgba", "kind", "shadowed")


@functools.lru_cache(maxsize=None)
def voxel_source(vx, which):
    """-> (voxels, (table, per-voxel ids) or None, the mesh to keep alive).  hidden: a small cube behind the sheet, which no primary ray that hits the sheet sees;
    slab: shading_extremes.slab() as a Bool grid with per-voxel materials; octree: the same slab as an octree (no materials: MaterialObj{})"""
    if which == "hidden":
        v, t = vx_scenes.cube(half=0.25, center=(0.0, 0.0, 3.0))
        return vx.Grid.voxelize(vx.Mesh.from_arrays(v, t), F(0.125)), None, None
    s = sx.slab()
    m = vx.Mesh.from_arrays(s.verts, s.tris)
    if which == "octree":
        return vx.Octree(m, s.voxel_size), None, m
    m.set_materials(s.mats, s.ids)
    g = vx.Grid.voxelize(m, s.voxel_size, materials=True)
    return g, g.materials(), m


@functools.lru_cache(maxsize=None)
def scene(vx, case_fn, arg, which):
    """the device objects of one sheet case, built once per process: mesh, bvh, the identity TLAS, the voxels, and the four renderers"""
    case = case_fn() if arg is None else case_fn(arg)
    vox, vmat, keep = voxel_source(vx, which)
    mesh = sx.build_mesh(vx, case.mesh)
    bvh = mesh.bvh()
    tl = vx.Tlas([bvh], vx.instances([instance_ref.transform()]))
    cam = case.sh.cam
    vo = vox.trace_ex(camera=cam, want=("t", "prim", "normal"))
    mo = bvh.trace_ex(camera=cam, want=("t", "prim", "normal", "bary"))
    r = {(a, False): vx.Renderer(vox, bvh, mesh, attributes=a) for a in MODES}
    r.update({(a, True): vx.Renderer.from_tlas(vox, tl, [mesh], attributes=a) for a in MODES})
    return sx._ns(case=case, vox=vox, vmat=vmat, mesh=mesh, bvh=bvh, tl=tl, cam=cam, vo=vo, mo=mo, r=r, keep=keep)


def run(vx, S, attributes, light=None, flat=None, what=None):
    """one case in one mode under one light: the BVH frame against the expectation, the identity-instance frame against the BVH frame"""
    case = S.case
    light = case.light if light is None else light
    what = "%s (%s)" % (what or case.name, "attributes" if attributes else "default")
    P = sx.prepare(S.cam, S.vo, S.mo, [case.mesh], light, attributes, S.vmat)
    sv = S.vox.trace_ex(P.rays, tmax_per_ray=P.tmax, any_hit=True, want=("shadowed",))["shadowed"]
    sm = S.bvh.trace_ex(P.rays, tmax_per_ray=P.tmax, any_hit=True, want=("shadowed",))["shadowed"]
    exp = sx.expected(P, sv, sm)
    st = sx.check_stats(exp, flat if flat is not None else case.flat, what)
    out = S.r[(attributes, False)].render_host(S.cam, light, want=WANT)
    res = sx.compare(out, exp, what=what)
    print("TIE %-60s max_tie %.3e differing %5d near_share %.5f distinct %3d" % (what, res["max_tie"], res["differing"], st["near_share"], st["distinct"]))
    inst = S.r[(attributes, True)].render_host(S.cam, light, want=WANT)
    for k in WANT:
        assert np.array_equal(out[k], inst[k]), "%s: the identity instance's %s differs from the BVH scene's" % (what, k)
    return P, exp, out


# ---- gamma and the sRGB table, directly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", MODES, ids=MODE_IDS)
def test_gamma_boundaries(gpu, attributes):
    S = scene(gpu, sx.case_gamma, None, "hidden")
    P, exp, out = run(gpu, S, attributes)
    tri = P.kind == 2
    assert tri.sum() > 32000 and not P.lit[tri].any()
    amb = S.case.ambient[sx.quad_of(S.mo["prim"][tri])]
    assert np.array_equal(exp["c"][tri], amb, equal_nan=True)                        # c IS the ambient: the pre-gamma colour is the input
    rgb = out["rgba"].reshape(-1, 4)[tri, :3]
    with np.errstate(invalid="ignore"):
        assert (rgb[np.isnan(amb)] == 0).all() and (rgb[amb == np.inf] == 255).all() and (rgb[amb < 0] == 0).all()
        assert (rgb[amb == 0] == 0).all() and (rgb[amb >= 1] == 255).all() and (rgb[amb == sx.SUBNORMAL] == 0).all()
    assert sx.tie_distance(exp["y"][tri]).min() >= 1.5 * sx.M_TIE                   # no channel of this frame is allowed any slack
    assert np.array_equal(rgb, exp["byte"][tri])


def test_srgb_table(gpu):
    S = scene(gpu, sx.case_srgb, None, "hidden")
    P, exp, out = run(gpu, S, True)
    tri = P.kind == 2
    assert not P.lit[tri].any() and np.array_equal(exp["c"][tri], P.tex[tri])        # ambient 1, unlit: c is the texture factor


# ---- texture addressing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sloped", [False, True], ids=["const", "sloped"])
def test_texture_addressing(gpu, sloped):
    S = scene(gpu, sx.case_texture, sloped, "hidden")
    P, exp, out = run(gpu, S, True)
    tri = np.flatnonzero(P.kind == 2)
    arms, _ = sx.texture_arms(S.case.mesh, S.mo["prim"][tri], S.mo["bary"][tri])
    for a in (0, 1, 2):
        assert (arms == a).any(1).sum() > 1000, a                                    # every arm of tex_axis runs on the device, on both axes
        assert (arms[:, 0] == a).sum() > 500 and (arms[:, 1] == a).sum() > 500


def test_texture_slots_and_material_ids(gpu):
    S = scene(gpu, sx.case_slots, None, "hidden")
    P, exp, out = run(gpu, S, True)
    ma = S.case.mesh
    with pytest.raises(gpu.VxError):                                                # an id equal to the table size never reaches the device
        S.mesh.set_materials(ma.mats, np.full(len(ma.ids), len(ma.mats), np.int32))
    with pytest.raises(gpu.VxError):
        S.mesh.set_materials(ma.mats, np.full(len(ma.ids), -2, np.int32))
    assert np.array_equal(S.mesh.materials()[1], ma.ids) and np.array_equal(S.mesh.material_textures(), ma.slots)   # ... and changes nothing
    for shape in ((1, 16385), (16385, 1)):                                           # one past the 16384 the texture case runs at
        with pytest.raises(gpu.VxError):
            S.mesh.set_texture(0, np.zeros(shape + (4,), np.uint8))
    assert S.mesh.texture(0).shape == ma.images[0].shape
    run(gpu, S, False)                                                               # the default mode reads no slot


# ---- normals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", [False, True, "tiny"], ids=["directional", "point", "tiny"])
def test_normal_fallbacks(gpu, point):
    S = scene(gpu, sx.case_normals, point, "hidden")
    P, exp, out = run(gpu, S, True)
    tri = np.flatnonzero(P.kind == 2)
    probe = sx.quad_of(S.mo["prim"][tri]) % 16
    for p, (name, _, falls) in enumerate(sx.NORMAL_PROBES):
        if falls is not None:
            assert P.fell[tri][probe == p].all() == falls and P.fell[tri][probe == p].any() == falls, name
    d = S.r[(False, False)].render_host(S.cam, S.case.light, want=WANT)
    fell = np.zeros(P.n, bool)
    fell[tri] = P.fell[tri]
    for k in WANT:                                                                   # a normal that falls back gives the default mode's pixel
        assert np.array_equal(out[k].reshape(P.n, -1)[fell], d[k].reshape(P.n, -1)[fell]), k
    if point == "tiny":                                                              # the lit pixels with an infinite L: a shadow ray that hits nothing
        inf_l = P.lit & ~np.isfinite(P.rays).all(1)
        assert inf_l.sum() > 100 and (P.dnl0[inf_l] == np.inf).all() and not out["shadowed"].ravel()[inf_l].any()
        assert (out["rgba"].reshape(-1, 4)[inf_l, :3] == 255).all()
    if point is False:
        perp = tri[probe == [n for n, _, _ in sx.NORMAL_PROBES].index("perpendicular to FRONT")]
        assert (P.dnl0[perp] == 0).all() and not P.lit[perp].any() and not out["shadowed"].ravel()[perp].any()


# ---- materials ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("voxels", ["slab", "octree"])
def test_materials(gpu, voxels, attributes):
    S = scene(gpu, sx.case_materials, None, voxels)
    P, exp, out = run(gpu, S, attributes, what="materials beside the %s" % voxels)
    assert (P.kind == 1).sum() > 1000 and (P.kind == 2).sum() > 4000 and exp["shadowed"].sum() > 100
    assert np.isnan(exp["c"][P.kind == 2]).any(1).sum() > 100                         # NaN channels (Ns NaN or Inf) reach the gamma
    if voxels == "slab":
        assert len(S.vmat[0]) == np.unique(sx.slab().ids).size == 30                 # per-voxel materials: the ones the slab uses


# ---- lights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(sx.LIGHTS))
def test_lights(gpu, name, attributes):
    S = scene(gpu, sx.case_materials, None, "slab")
    P, exp, out = run(gpu, S, attributes, sx.LIGHTS[name], sx.FLAT_LIGHTS.get(name), what=name)
    finite = S.r[(attributes, False)].render_host(S.cam, sx.LIGHTS["directional"], want=WANT)
    assert np.array_equal(out["kind"], finite["kind"])                               # kind never depends on the light
    hit = P.kind > 0
    if name in sx.NAN_DOT_LIGHTS:
        assert np.isnan(P.dnl0[hit]).all() and not out["shadowed"].any()
    lit = P.lit & hit
    assert np.isfinite(P.rays[lit]).all() and np.isfinite(P.tmax[lit]).all()         # a lit pixel has a finite shadow ray


@pytest.mark.parametrize("attributes", MODES, ids=MODE_IDS)
def test_light_on_a_pixels_hit_point(gpu, attributes):
    S = scene(gpu, sx.case_materials, None, "slab")
    P0 = sx.prepare(S.cam, S.vo, S.mo, [S.case.mesh], sx.POINT, attributes, S.vmat)
    sh = S.case.sh
    px = (sh.H // 2 + 3) * sh.W + 3 * sh.W // 4 + 2                                    # a triangle pixel away from the slab
    light = sx.light_on_pixel(P0, px)
    P, exp, out = run(gpu, S, attributes, light, what="light on pixel %d" % px)
    assert np.isnan(P.dnl0[px]) and np.isnan(P.dnl0).sum() == 1 and not P.lit[px] and out["shadowed"].ravel()[px] == 0


# ---- instances ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def instanced_scene(vx):
    c = sx.case_instanced()
    meshes = [sx.build_mesh(vx, m) for m in c.meshes]
    blas = [m.bvh() for m in meshes]
    tl = vx.Tlas(blas, c.inst)
    vox, _, _ = voxel_source(vx, "hidden")
    mo = tl.trace_ex(camera=c.cam, want=("t", "instance", "prim", "bary", "normal"))
    vo = vox.trace_ex(camera=c.cam, want=("t", "prim", "normal"))
    r = {a: vx.Renderer.from_tlas(vox, tl, meshes, attributes=a) for a in MODES}
    return sx._ns(case=c, meshes=meshes, blas=blas, tl=tl, vox=vox, mo=mo, vo=vo, r=r)


@pytest.mark.parametrize("attributes", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("light", ["point", "directional"])
def test_scaled_mirrored_instance_beside_other_blas(gpu, light, attributes):
    S = instanced_scene(gpu)
    c = S.case
    lt = sx.POINT if light == "point" else sx.FRONT
    what = "instanced %s (%s)" % (light, "attributes" if attributes else "default")
    P = sx.prepare(c.cam, S.vo, S.mo, c.meshes, lt, attributes, None, c.inst, S.tl.world_to_object())
    sv = S.vox.trace_ex(P.rays, tmax_per_ray=P.tmax, any_hit=True, want=("shadowed",))["shadowed"]
    sm = S.tl.trace_ex(P.rays, tmax_per_ray=P.tmax, any_hit=True, want=("shadowed",))["shadowed"]
    exp = sx.expected(P, sv, sm)
    st = sx.check_stats(exp, None, what)
    out = S.r[attributes].render_host(c.cam, lt, want=WANT)
    res = sx.compare(out, exp, what=what)
    print("TIE %-60s max_tie %.3e differing %5d near_share %.5f distinct %3d" % (what, res["max_tie"], res["differing"], st["near_share"], st["distinct"]))
    tri = P.kind == 2
    for b in range(3):
        assert (c.inst["blas"][S.mo["instance"][tri].astype(np.int64)] == b).sum() > 3000, b
