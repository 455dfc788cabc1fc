"""CPU tests of the distance fields: the numpy restatement (tests/distance_ref.py) against the definition and against scipy, its C
helper against the numpy form, the cross-compiled library's exports and NULL-grid check, the correctly rounded square root in the
kernel's ISA, and the CLI's refusals of --sdf (all of them run before any device is touched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distance_ref
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")

# every size from 1 to 9 on every axis
DIMS = [(a, (a * 4) % 9 + 1, (a * 7) % 9 + 1) for a in range(1, 10)]
DIMS += [(z, x, y) for (x, y, z) in DIMS] + [(y, z, x) for (x, y, z) in DIMS]


@pytest.mark.parametrize("dims", DIMS)
def test_restatement_matches_brute_force(dims):
    rng = np.random.default_rng(sum(dims) * 31 + dims[0])
    X, Y, Z = dims
    for p in (0.0, 0.08, 0.5, 1.0):
        m = rng.random((Z, Y, X)) < p
        for target in (m, ~m):
            want = distance_ref.brute_sq(target)
            assert np.array_equal(distance_ref.edt_sq(target), want), (dims, p)
            assert np.array_equal(distance_ref.edt_sq_c(target), want), (dims, p)


def test_empty_and_full_masks_give_the_sentinel():
    m = np.zeros((3, 4, 5), bool)
    assert (distance_ref.edt_sq(m) == 0xFFFFFFFF).all() and (distance_ref.edt_sq_c(m) == 0xFFFFFFFF).all()
    w = distance_ref.pack(~m)
    assert (distance_ref.distance_sq(w, (5, 4, 3), inside=True) == 0xFFFFFFFF).all()
    assert (distance_ref.distance_sq(w, (5, 4, 3)) == 0).all()
    s = distance_ref.sdf(w, (5, 4, 3), 0.5)
    assert s.dtype == np.float32 and (s == -np.inf).all()
    s = distance_ref.sdf(distance_ref.pack(m), (5, 4, 3), 0.5)
    assert (s == np.inf).all()


def test_sdf_formula_and_signs():
    m = np.zeros((1, 1, 6), bool)
    m[0, 0, 2:4] = True
    s = distance_ref.sdf(distance_ref.pack(m), (6, 1, 1), 0.25)
    vs = np.float32(0.25)
    want = np.array([vs * np.sqrt(np.float32(4)), vs, -vs, -vs, vs, vs * np.sqrt(np.float32(4))], np.float32)
    assert s.reshape(-1).tobytes() == want.tobytes()
    assert (s != 0).all()


@pytest.mark.parametrize("shape,p", [((13, 17, 19), 0.01), ((8, 40, 33), 0.3), ((31, 5, 64), 0.002)])
def test_restatement_matches_scipy(shape, p):
    nd = pytest.importorskip("scipy.ndimage")
    m = np.random.default_rng(7).random(shape) < p
    m[0, 0, 0] = True
    m[-1, -1, -1] = False
    for target in (m, ~m):
        e = np.rint(nd.distance_transform_edt(~target) ** 2).astype(np.uint32)
        assert np.array_equal(distance_ref.edt_sq(target), e)


def test_c_helper_matches_numpy_on_larger_masks():
    rng = np.random.default_rng(3)
    for shape, p in (((20, 30, 70), 0.001), ((50, 3, 41), 0.2), ((1, 1, 3000), 0.001), ((200, 2, 2), 0.01)):
        m = rng.random(shape) < p
        for target in (m, ~m):
            assert np.array_equal(distance_ref.edt_sq_c(target), distance_ref.edt_sq(target)), shape


def test_library_exports_the_distance_entry_points(vx):
    L = ctypes.CDLL(vx.LIB_PATH)
    for n in ("vx_grid_distance_sq_device", "vx_grid_distance_sq", "vx_grid_sdf_device", "vx_grid_sdf"):
        assert hasattr(L, n) and n in vx.SYMBOLS, n
    assert vx.DISTANCE_INSIDE == 1


def test_null_grid_is_invalid(vx):
    L = vx.lib()
    buf = np.zeros(8, np.uint32)
    assert L.vx_grid_distance_sq(None, 0, buf.ctypes.data, 8) == 1
    assert L.vx_grid_distance_sq_device(None, 0, buf.ctypes.data, 8) == 1
    f = np.zeros(8, np.float32)
    assert L.vx_grid_sdf(None, f.ctypes.data, 8) == 1
    assert L.vx_grid_sdf_device(None, f.ctypes.data, 8) == 1
    assert (buf == 0).all() and (f == 0).all()


def test_sqrt_is_correctly_rounded_in_the_isa(tmp_path):
    """The signed field's sqrtf must be the correctly rounded expansion (v_sqrt_f32 followed by the fma checks of its two neighbours),
    not a bare v_sqrt_f32 (1 ulp)."""
    import build as vxbuild
    if not os.path.exists(vxbuild.HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path / "d.s"
    subprocess.check_call([vxbuild.HIPCC] + vxbuild.FLAGS + ["--cuda-device-only", "-S", "-x", "hip",
                                                             os.path.join(vxbuild.CSRC, "vx_distance.hip"), "-o", str(out)])
    asm = out.read_text()
    body = [b for b in asm.split("\n_Z") if b.startswith("N2vx12_GLOBAL__N_110k_dist_colILi2ELb1E")]
    assert len(body) == 1
    lines = [ln.strip() for ln in body[0].split("s_endpgm")[0].splitlines()]
    at = [i for i, ln in enumerate(lines) if ln.startswith("v_sqrt_f32")]
    assert len(at) == 1, "expected one square root in the converting pass"
    after = lines[at[0]:at[0] + 16]
    assert sum(ln.startswith("v_fma_f32") for ln in after) >= 2, "\n".join(after)
    assert "v_rsq_f32" not in body[0]


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["--grid", "octree"], ["--gpus", "2"], ["--bench", "2"]])
def test_cli_sdf_refusals(built, tmp_path, extra):
    obj = tmp_path / "c.obj"
    v, t = vx_scenes.cube()
    vx_scenes.write_obj(str(obj), v, t)
    r = run_cli([str(obj), "0.25", "--sdf", str(tmp_path / "f.bin")] + extra)
    assert r.returncode == 2 and "--sdf writes the distance field of one grid on one device" in r.stdout, r.stdout
    assert not (tmp_path / "f.bin").exists()
