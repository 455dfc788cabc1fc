"""The references on geometry at its extremes (tests/geometry_extremes.py), on the host: what makes tests/test_gpu_geometry_extremes.py mean
something.  The Moeller-Trumbore brute forces accept no triangle that has a non-finite vertex and do accept triangles that reach to a far
finite vertex; the voxelizer oracle's result changes with the scale 2^k of the scene exactly as recorded (and the pinned build of the
reference's own sources says the same); and the OBJ reader reads numerals at and beyond the edges of double and float as Python's float()
does -- through the library's own entry points and once more as a stand-alone program under UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import geometry_extremes as gx
import instance_ref
import mesh_multihit_ref as mmr
import mesh_ref
import reference_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
F = np.float32
K = 4
POISONS = [(k, v) for k in gx.POISON_KINDS for v in gx.POISON_BITS]


def cpu_rays(name):
    """base_rays + the zero-component rays of the scene; every 4th of them on the 2317-triangle scene (the brute force is rays x triangles)"""
    r = gx.mesh_rays(name)[:2400]
    return r[::4] if name == "adversarial" else r


_clean = {}


def clean_results(name):
    if name not in _clean:
        v, t = gx.scene(name)
        rays = cpu_rays(name)
        _clean[name] = (mesh_ref.closest(v, t, rays), mesh_ref.any_hit(v, t, rays), mmr.select(mmr.all_hits(v, t, rays), K))
    return _clean[name]


@pytest.mark.parametrize("name", gx.SCENES)
def test_references_accept_no_poisoned_triangle(name):
    rays = cpu_rays(name)
    (ct, cp, cb), cany, cmulti = clean_results(name)
    assert (ct > 0).mean() > 0.1
    for kind, value in POISONS:
        m = gx.poisoned(name, kind, value)
        what = "%s %s %s" % (name, kind, value)
        assert m.stray.sum() >= 2 and not np.isfinite(m.v[m.t[m.stray]]).all(axis=(1, 2)).any(), what
        hits = mmr.all_hits(m.v, m.t, rays)
        assert not m.stray[hits.prim].any(), what                                   # the brute force accepts no such triangle, on any ray
        t, p, b = mesh_ref.closest(m.v, m.t, rays)
        assert gx.rx.same_bits(t, ct) and np.array_equal(gx.remap_prim(p, m.remap), cp) and gx.rx.same_bits(b, cb), what
        assert np.array_equal(mesh_ref.any_hit(m.v, m.t, rays), cany), what
        multi = mmr.select(hits, K)
        assert gx.rx.same_bits(multi["t"], cmulti["t"]) and np.array_equal(multi["count"], cmulti["count"]), what
        assert np.array_equal(gx.remap_prim(multi["prim"], m.remap), cmulti["prim"]) and gx.rx.same_bits(multi["bary"], cmulti["bary"]), what


def test_instance_ref_accepts_no_poisoned_triangle():
    """the same through instance_ref: two instances (one rotated and scaled) of the poisoned floor against the same of the clean one"""
    name = "floor"
    rays = cpu_rays(name)
    rng = np.random.default_rng(5)
    tr = [instance_ref.transform(np.eye(3)), instance_ref.transform(instance_ref.random_rotation(rng), (1.5, 0.5, 2.0), 0.0, (0.5, 1.0, -0.5))]
    inst = instance_ref.make_instances(tr)
    v, t = gx.scene(name)
    ct, ci, cp, cb = instance_ref.closest([(v, t)], inst, rays)
    cm = mmr.select(mmr.all_hits_tlas([(v, t)], inst, rays), K)
    for kind, value in POISONS:
        m = gx.poisoned(name, kind, value)
        hits = mmr.all_hits_tlas([(m.v, m.t)], inst, rays)
        assert not m.stray[hits.prim].any(), (kind, value)
        tt, ii, pp, bb = instance_ref.closest([(m.v, m.t)], inst, rays)
        assert gx.rx.same_bits(tt, ct) and np.array_equal(ii, ci) and np.array_equal(gx.remap_prim(pp, m.remap), cp) and gx.rx.same_bits(bb, cb), (kind, value)
        mm = mmr.select(hits, K)
        assert gx.rx.same_bits(mm["t"], cm["t"]) and np.array_equal(gx.remap_prim(mm["prim"], m.remap), cm["prim"]) and np.array_equal(mm["count"], cm["count"])


@pytest.mark.parametrize("mag", gx.OUTLIERS)
@pytest.mark.parametrize("name", gx.BVH_SCENES)
def test_references_reach_the_outliers(name, mag):
    """a finite far vertex is ordinary input: the brute force accepts triangles that reach to it, so the GPU has something to get right"""
    m = gx.outlier(name, mag)
    rays = gx.mesh_rays(name)
    hits = mmr.all_hits(m.v, m.t, rays)
    n = int(m.stray[hits.prim].sum())
    print(name, mag, "accepted (ray, stray) pairs:", n, "distinct strays:", len(np.unique(hits.prim[m.stray[hits.prim]])))
    assert n >= 1
    for far in range(m.first_new, len(m.v)):                                        # ... to EACH far vertex (fltmax: the +FLT_MAX/2 and the -FLT_MAX/2 one)
        assert (m.t[hits.prim] == far).any(), (name, mag, far)
    t, p, b = mesh_ref.closest(m.v, m.t, rays)
    assert m.stray[p[p != mesh_ref.MISS].astype(np.int64)].any()                      # ... and some are the closest hit
    sc = gx.outlier_tlas(name, mag)
    th = mmr.all_hits_tlas(sc.meshes, sc.inst, gx.tlas_rays(name))
    on_outlier = (sc.inst["blas"][th.inst] == 0)
    assert m.stray[th.prim[on_outlier]].any() and (~on_outlier).any()
    # the unreferenced variant is the clean mesh with vertices nobody uses
    u = gx.outlier(name, mag, referenced=False)
    assert np.array_equal(u.t, u.clean_t) and len(u.v) > len(u.clean_v)


@pytest.mark.parametrize("sat", [1, 0])
@pytest.mark.parametrize("name", gx.GRID_SCENES)
def test_oracle_changes_with_scale_as_recorded(name, sat):
    table = gx.ORACLE_TABLE[name, sat]
    assert set(gx.SCALE_K[sat]) <= set(table)
    dims = gx.oracle_counts(name, sat, 0)[2]
    for k, want in table.items():
        calls, occ, d = gx.oracle_counts(name, sat, k)
        assert (calls, occ) == want and d == dims, (name, sat, k, calls, occ, d)
    dk = gx.DISTINCT_K[name, sat]
    assert len({table[k][0] for k in dk}) == len(dk)
    for k in gx.SCALE_K[sat]:
        assert gx.scaled(name, k).exact or (name == "adversarial" and k == -100)


@pytest.fixture(scope="module")
def vxref():
    if not rc.build_ref():
        pytest.skip("no reference voxelizer: neither the reference sources (VOXHIP_REFERENCE_DIR=%s) nor a built %s exist" % (rc.REFERENCE_DIR, rc.VXREF))
    return rc.VXREF


@pytest.mark.parametrize("name", gx.GRID_SCENES)
def test_pinned_reference_changes_with_scale_the_same_way(vxref, tmp_path, name):
    """the reference's own voxelizer on the scaled OBJ: serial driver = sat 0, threaded driver = sat 1; Vec entries = setVoxel calls"""
    for sat, modes in ((0, ("bool", "vec")), (1, ("bool_par", "vec_par"))):
        for k in gx.SCALE_K[sat]:
            s = gx.scaled(name, k)
            obj = tmp_path / ("%s_%d.obj" % (name, k))
            if not obj.exists():
                rc.write_obj(obj, s.v, s.t)
            calls, occ = gx.ORACLE_TABLE[name, sat][k]
            r = rc.run_vxref(obj, s.vs, modes[0], tmp_path / "b")
            assert int(np.unpackbits(r["occ"].view(np.uint8)).sum()) == occ == len(r["aabbs"]), (name, sat, k)
            assert len(rc.run_vxref(obj, s.vs, modes[1], tmp_path / "v")["aabbs"]) == calls, (name, sat, k)


# ---- OBJ numerals -------------------------------------------------------------------------------------------------------------------------
def write_obj_case(d):
    obj, mtl, verts, (kd, ns) = gx.obj_texts()
    (d / "scene.obj").write_text(obj)
    (d / "scene.mtl").write_text(mtl)
    return str(d / "scene.obj"), verts, kd, ns


def test_obj_numerals_through_the_library(built, tmp_path):
    """vx_mesh_load_obj + vx_mesh_host_vertices / vx_mesh_materials (no device) against Python's float() -> float32 of every numeral"""
    import voxhip
    path, verts, kd, ns = write_obj_case(tmp_path)
    m = voxhip.Mesh.load_obj(path)
    v, t = m.host_arrays()
    assert v.shape == verts.shape and len(t) == 1
    bad = [i for i in range(len(v)) if not gx.same_f32(v[i], verts[i])]
    assert not bad, "vertex lines %s: read %s, float() says %s" % (bad[:4], v[bad[:4]].tolist(), verts[bad[:4]].tolist())
    recs, ids = m.materials()
    assert len(recs) == len(gx.NUMERALS) and ids is not None and ids[0] == 0
    for i, s in enumerate(gx.NUMERALS):
        assert gx.same_f32(recs["diffuse"][i], kd[i]), (s, recs["diffuse"][i], kd[i])
        assert gx.same_f32(recs["shininess"][i], ns[i]), (s, recs["shininess"][i], ns[i])
        assert gx.same_f32(recs["specular"][i], F([0.5, 0.25, i + 3])), s
    # the numerals that carry the rules: beyond double -> +-Inf, below it -> +-0 with the numeral's sign, beyond float -> +-Inf
    col = {s: verts[1 + 6 * i, 0] for i, s in enumerate(gx.NUMERALS)}
    assert col["1e999"] == np.inf and col["-1e999"] == -np.inf and col["1e300"] == np.inf and col["-1e300"] == -np.inf
    assert col["1e-999"] == 0 and not np.signbit(col["1e-999"]) and col["-1e-999"] == 0 and np.signbit(col["-1e-999"])
    assert np.isnan(col["nan"]) and col["-inf"] == -np.inf and col["+1.5"] == 1.5 and col[".5e+1"] == 5.0
    m.free()


MAIN = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "voxhip.h"
#include "vx_obj.h"
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::vector<float> verts; std::vector<int32_t> tris, tri_mat; std::vector<vx_material> mats; std::string msg;
    vx::ObjAttributes attr;
    const int rc = vx::load_obj(argv[1], verts, tris, tri_mat, mats, msg, &attr);
    if (rc) { std::printf("ERROR %d %s\n", rc, msg.c_str()); return 1; }
    for (size_t i = 0; i < verts.size(); i += 3) {
        uint32_t b[3]; std::memcpy(b, &verts[i], 12);
        std::printf("V %08x %08x %08x\n", b[0], b[1], b[2]);
    }
    for (const vx_material& m : mats) {
        uint32_t b[4]; std::memcpy(b, m.diffuse, 12); std::memcpy(b + 3, &m.shininess, 4);
        std::printf("M %08x %08x %08x %08x\n", b[0], b[1], b[2], b[3]);
    }
    return 0;
}
"""


def test_obj_reader_stand_alone_under_sanitizers(tmp_path):
    """the same reader with a main of its own under UndefinedBehaviorSanitizer and the float-cast-overflow check (host build, the runtime
    linked into the program), once, on the same files"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    ubsan = subprocess.check_output(["g++", "-print-file-name=libubsan.a"]).decode().strip()
    if not (os.path.isabs(ubsan) and os.path.exists(ubsan)):
        pytest.skip("g++ sanitizer runtime not installed")
    path, verts, kd, ns = write_obj_case(tmp_path)
    src = tmp_path / "obj_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "obj_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"), "-o", exe, str(src), os.path.join(PKG, "csrc", "vx_obj.cpp")])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    rows = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("V ")]
    got = np.array([[int(x, 16) for x in row] for row in rows], np.uint32).view(F)
    assert got.shape == verts.shape and all(gx.same_f32(got[i], verts[i]) for i in range(len(verts))), r.stdout[:2000]
    mrows = np.array([[int(x, 16) for x in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("M ")], np.uint32).view(F)
    assert len(mrows) == len(gx.NUMERALS)
    assert all(gx.same_f32(mrows[i, :3], kd[i]) and gx.same_f32(mrows[i, 3], ns[i]) for i in range(len(kd)))
