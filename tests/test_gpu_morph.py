"""GPU tests of the morphology (vx_grid_morph*, vx_grid_seal): every result is compared whole, word for word, with the numpy restatements
(tests/morph_ref.py) of the mask the GPU itself holds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import morph_ref as mr
import oracle
import solid_ref
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
OPS = [mr.DILATE, mr.ERODE, mr.OPEN, mr.CLOSE]
OP_NAMES = {mr.DILATE: "dilate", mr.ERODE: "erode", mr.OPEN: "open", mr.CLOSE: "close"}
ORIGIN = (0.25, -1.0, 3.0)


def masked_grid(gpu, cells, kind=None, vs=F(0.5), dirty_tail=False):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, vs, ORIGIN)
    w = solid_ref.pack(cells).copy()
    if dirty_tail and (X * Y * Z) % 32:
        w[-1] |= np.uint32(0xFFFFFFFF) << np.uint32((X * Y * Z) % 32)  # padding bits are not cells: refresh() clears them
    write_mask(g, w)
    g.refresh()
    return g


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).sum())


# ---- small shapes, every operation, both sides of every word boundary ---------------------------------------------------------------
DIMS = [(37, 9, 7), (64, 33, 5), (70, 1, 1), (31, 3, 12), (7, 2, 40)]   # X, Y, Z
R2S = [0, 1, 2, 3, 4, 5, 6, 8, 9, 14, 27]


def small_masks(dims):
    X, Y, Z = dims
    shape = (Z, Y, X)
    rng = np.random.default_rng(X * 131 + Y * 17 + Z)
    empty, full = np.zeros(shape, bool), np.ones(shape, bool)
    corner, centre = empty.copy(), empty.copy()
    corner[0, 0, 0] = True
    centre[Z // 2, Y // 2, X // 2] = True
    return [("empty", empty), ("full", full), ("corner", corner), ("centre", centre)] + [("random %g" % d, rng.random(shape) < d) for d in (0.02, 0.5, 0.98)]


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("op", OPS)
def test_small_shapes(gpu, dims, op):
    assert max(mr.radius(r2) for r2 in R2S) <= gpu.morph_bit_radius()
    for k, (name, cells) in enumerate(small_masks(dims)):
        g = masked_grid(gpu, cells, dirty_tail=(k == 6))
        assert np.array_equal(g.bitmask(), solid_ref.pack(cells))
        for r2 in R2S:
            want = solid_ref.pack(mr.apply(op, cells, r2))
            got = g.morph_mask(op, r2)
            assert np.array_equal(got, want), "%s %s r2=%d dims=%s: %d words differ" % (OP_NAMES[op], name, r2, dims, int((got != want).sum()))
        if name == "centre" and op == mr.DILATE:   # exactly the clipped ball
            Z, Y, X = cells.shape
            z, y, x = np.ogrid[:Z, :Y, :X]
            ball = (x - X // 2) ** 2 + (y - Y // 2) ** 2 + (z - Z // 2) ** 2 <= 14
            assert np.array_equal(g.morph_mask(op, 14), solid_ref.pack(ball))


def test_device_variant_and_stream(gpu):
    import torch
    cells = np.random.default_rng(5).random((9, 11, 45)) < 0.1
    st = torch.cuda.Stream()
    g = gpu.Grid.create(gpu.GRID_BOOL, 45, 11, 9, F(0.5), ORIGIN, stream=st.cuda_stream)
    write_mask(g, solid_ref.pack(cells))
    g.refresh()
    n = g.describe()["num_words"]
    for op in OPS:
        with torch.cuda.stream(st):
            out = g.morph_mask_device(op, 5)
            big = torch.full((n + 3,), 0x1234567, dtype=torch.int32, device="cuda")
            g.morph_mask_device(op, 5, out=big)
        st.synchronize()
        want = solid_ref.pack(mr.apply(op, cells, 5))
        assert out.dtype == torch.uint32 and out.numel() == n
        assert np.array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), want)
        b = big.cpu().numpy()
        assert np.array_equal(b[:n].view(np.uint32), want) and (b[n:] == 0x1234567).all()
    assert np.array_equal(g.bitmask(), solid_ref.pack(cells))


# ---- both sides of the crossover ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [mr.DILATE, mr.ERODE, mr.CLOSE])
def test_both_sides_of_the_crossover(gpu, op):
    R = gpu.morph_bit_radius()
    rng = np.random.default_rng(40 + op)
    shape = (33, 37, 40)
    if op == mr.ERODE:  # full but for a few cells: a large ball leaves little, the holes decide what
        cells = np.ones(shape, bool)
        Z, Y, X = shape
        for z, y, x in ((0, 0, 0), (Z // 2 + 2, Y // 2 + 7, X // 2 + 10), (Z - 1, 3, X // 2)):
            cells[z, y, x] = False
    else:
        cells = rng.random(shape) < 2e-4
        cells[16, 18, 20] = True
    g = masked_grid(gpu, cells)
    for radius, bit in ((R, True), (R + 1, False)):
        for r2 in (radius * radius, (radius + 1) ** 2 - 1):
            gpu.profile_enable(True)
            gpu.profile_reset()
            got = g.morph_mask(op, r2)
            names = list(gpu.profile_read())
            gpu.profile_enable(False)
            want = solid_ref.pack(mr.apply_fast(op, cells, r2, c=True))
            assert np.array_equal(got, want), "%s r2=%d: %d words differ" % (OP_NAMES[op], r2, int((got != want).sum()))
            assert any("k_dist_col" in n for n in names) == (not bit), (r2, names)
            assert any("k_morph_ball" in n for n in names) == (bit or op == mr.CLOSE), (r2, names)


# ---- built grids: the result as a grid ----------------------------------------------------------------------------------------------
BUILT = {}


def built_case(gpu, name, vs):
    """the oracle's mask of the scene and, computed once, the expected mask of every operation tried on it"""
    key = (name, float(vs))
    if key not in BUILT:
        v, t = vx_scenes.scene(name)
        ow, calls, gi = oracle.build_bool(v, t, vs)
        m = solid_ref.unpack(ow, gi["dim"])
        exp = {("morph", op, r2): mr.apply_fast(op, m, r2, c=True) for op, r2 in ((mr.DILATE, 3), (mr.ERODE, 1), (mr.OPEN, 2), (mr.CLOSE, 5))}
        exp[("seal", None, 2)] = mr.seal_fast(m, 2, c=True)
        BUILT[key] = (v, t, ow, gi, m, exp)
    return BUILT[key]


def check_result_grid(gpu, r, src_desc, cells, kind, gi, vs):
    words = solid_ref.pack(cells)
    n = int(cells.sum())
    d = r.describe()
    assert d["dim"] == src_desc["dim"] and d["kind"] == kind and d["voxel_size"] == src_desc["voxel_size"]
    for k in ("origin", "bbox_min", "bbox_max", "bbox_center"):
        assert np.array_equal(d[k], src_desc[k]), k
    assert d["occupied"] == n and d["set_calls"] == n and d["triangles"] == 0
    assert np.array_equal(r.bitmask(), words)
    assert r.aabbs().tobytes() == oracle.bool_aabbs(words, gi, vs).tobytes()
    N = int(np.prod(gi["dim"]))
    assert r.memory_bytes() == {gpu.GRID_BOOL: 4 * ((N + 31) // 32), gpu.GRID_AABBSTRUCT: 28 * N, gpu.GRID_VEC: 24 * n}[kind]
    assert len(r.materials()[0]) == 0


@pytest.mark.parametrize("name,vs", [("rotcube", 0.09), ("blob70k", 2.0 / 97)])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_built_grids(gpu, name, vs, kind):
    vs = F(vs)
    v, t, ow, gi, m, exp = built_case(gpu, name, vs)
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), vs, kind)
    d0, w0, a0 = g.describe(), g.bitmask(), g.aabbs()
    assert np.array_equal(w0, ow)
    for (what, op, r2), cells in exp.items():
        r = g.seal(radius_sq=r2) if what == "seal" else g._morph_grid(op, None, r2)
        check_result_grid(gpu, r, d0, cells, kind, gi, vs)
        assert r.interior() == (int(cells.sum()) - int(m.sum()) if what == "seal" else 0)
        r.free()
    # the result is a grid like any other: morph it again, fill it, label it, trace it
    r = g.close(radius=1.5)
    assert np.array_equal(r.bitmask(), solid_ref.pack(mr.close(m, 2)))
    c2 = mr.close(m, 2)
    assert np.array_equal(r.erode(radius=1).bitmask(), solid_ref.pack(mr.erode(c2, 1)))
    assert np.array_equal(r.distance_sq(), mr.distance_ref.edt_sq_c(c2))
    nh = r.fill_interior()
    assert nh == int(solid_ref.interior_cells(c2).sum()) and r.components()[1] >= 1
    rays = vx_scenes.random_rays(512, gi["bmin"], gi["bmax"], seed=3)
    tt, pp, _ = r.trace(rays)
    ot, op_ = oracle.trace_brute(r.aabbs() if kind != gpu.GRID_VEC else oracle.bool_aabbs(r.bitmask(), gi, vs), rays)
    assert np.array_equal(tt > 0, ot > 0) and np.allclose(tt, ot, rtol=0, atol=1e-5)
    # and the source is untouched
    d1 = g.describe()
    assert all(np.array_equal(d0[k], d1[k]) for k in d0) and np.array_equal(g.bitmask(), w0) and g.aabbs().tobytes() == a0.tobytes()


def test_source_with_pending_async_list_is_untouched(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    vs = F(2.0 / 64)
    a = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)
    b = gpu.Grid.voxelize(mesh, vs, gpu.GRID_VEC)
    a.revoxelize(mesh, vs, list_async=True)
    b.revoxelize(mesh, vs, list_async=True)
    m = solid_ref.unpack(b.bitmask(), b.describe()["dim"])
    r = b.dilate(radius=1)
    s = b.seal(radius=1)
    w = b.morph_mask(gpu.MORPH_OPEN, 1)
    b.morph_mask_device(gpu.MORPH_CLOSE, 2)
    assert np.array_equal(r.bitmask(), solid_ref.pack(mr.dilate_fast(m, 1, c=True))) and np.array_equal(w, solid_ref.pack(mr.open_fast(m, 1, c=True)))
    assert np.array_equal(s.bitmask(), solid_ref.pack(mr.seal_fast(m, 1, c=True)))
    da, db = a.describe(), b.describe()
    assert all(np.array_equal(da[k], db[k]) for k in da) and np.array_equal(a.bitmask(), b.bitmask())
    assert a.aabbs().tobytes() == b.aabbs().tobytes() and a.memory_bytes() == b.memory_bytes()


# ---- the leaky mesh -----------------------------------------------------------------------------------------------------------------
def test_holed_box_seal(gpu):
    v, t = vx_scenes.holed_box(0.6)
    vs = F(0.1)
    ow, _, gi = oracle.build_bool(v, t, vs)
    m = solid_ref.unpack(ow, gi["dim"])
    mesh = gpu.Mesh.from_arrays(v, t)
    g = gpu.Grid.voxelize(mesh, vs, gpu.GRID_BOOL, solid=True)
    assert g.interior() == 0 and np.array_equal(g.bitmask(), ow)
    sealed = {}
    for r2 in (4, 5):
        s = g.seal(radius_sq=r2)
        want = mr.seal_fast(m, r2, c=True)
        assert np.array_equal(s.bitmask(), solid_ref.pack(want)), r2
        assert s.interior() == int(want.sum()) - int(m.sum()) == s.describe()["occupied"] - g.describe()["occupied"]
        sealed[r2] = (s, want)
    assert sealed[4][0].interior() < 1000 < sealed[5][0].interior()
    # a ray along x through the box's centre, accepted from just before the centre on: the sealed grid answers with an interior voxel
    ray = np.array([[-5.0, 0.013, 0.021, 1.0, 0.0, 0.0]], np.float32)
    s5, want5 = sealed[5]
    t5, p5, _ = s5.trace(ray, tmin=4.9)
    t0, p0, _ = g.trace(ray, tmin=4.9)
    assert t5[0] > 0 and t0[0] > t5[0]
    cell = int(np.flatnonzero(want5.reshape(-1))[int(p5[0])])
    assert not m.reshape(-1)[cell], "the hit voxel exists only in the sealed grid"


# ---- mid-size ---------------------------------------------------------------------------------------------------------------------
def test_blob_256_dilate(gpu):
    v, t = vx_scenes.blob()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 256), gpu.GRID_BOOL)
    d = g.describe()
    assert max(d["dim"]) >= 250
    m = solid_ref.unpack(g.bitmask(), d["dim"])
    assert np.array_equal(g.morph_mask(gpu.MORPH_DILATE, 9), solid_ref.pack(mr.dilate_fast(m, 9, c=True)))


def test_blob_96_close_on_the_distance_path(gpu):
    v, t = vx_scenes.blob()
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(v, t), F(2.0 / 96), gpu.GRID_BOOL)
    d = g.describe()
    R = gpu.morph_bit_radius() + 2
    m = solid_ref.unpack(g.bitmask(), d["dim"])
    want = mr.close_fast(m, R * R + 1, c=True)
    assert np.array_equal(g.morph_mask(gpu.MORPH_CLOSE, R * R + 1), solid_ref.pack(want))
    assert want.sum() > m.sum()


# ---- steady state ---------------------------------------------------------------------------------------------------------------------
def test_steady_state(gpu):
    import torch
    cells = np.random.default_rng(8).random((20, 21, 50)) < 0.05
    live0 = gpu.device_live_blocks()
    g = masked_grid(gpu, cells)
    R = gpu.morph_bit_radius()
    out = torch.empty(g.describe()["num_words"], dtype=torch.int32, device="cuda")
    for op in OPS:
        for r2 in (3, (R + 1) ** 2):
            g.morph_mask_device(op, r2, out=out)
            n0 = gpu.device_allocations()
            g.morph_mask_device(op, r2, out=out)
            g.morph_mask_device(op, r2, out=out)
            assert gpu.device_allocations() == n0, "a repeated call at the same size and radius allocated (%s, r2=%d)" % (OP_NAMES[op], r2)
    torch.cuda.synchronize()
    results = [g.dilate(radius=2), g.seal(radius=1), g.close(radius_sq=(R + 1) ** 2)]
    for r in results:
        r.free()
    g.free()
    assert gpu.device_live_blocks() == live0


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(gpu):
    import torch
    cells = np.random.default_rng(4).random((5, 6, 7)) < 0.2
    g = masked_grid(gpu, cells)
    L = gpu.lib()
    n = g.describe()["num_words"]
    host = np.full(n + 1, 0x12345678, np.uint32)
    dev = torch.full((n + 1,), 0x1234567, dtype=torch.int32, device="cuda")
    for fn, buf in ((L.vx_grid_morph_mask, host.ctypes.data), (L.vx_grid_morph_device, dev.data_ptr())):
        assert fn(g.h, 4, 1, buf, n) == INVALID_ARG
        assert fn(g.h, 0, 0xFFFFFFFF, buf, n) == INVALID_ARG
        assert fn(g.h, 0, 1, None, n) == INVALID_ARG
        assert fn(None, 0, 1, buf, n) == INVALID_ARG
        assert fn(g.h, 0, 1, buf, n - 1) == CAPACITY
        assert fn(g.h, 3, (gpu.morph_bit_radius() + 1) ** 2, buf, n - 1) == CAPACITY
    w0 = g.bitmask()
    own = g.bitmask_device_ptr()
    assert L.vx_grid_morph_device(g.h, 0, 1, own, n) == INVALID_ARG
    assert L.vx_grid_morph_device(g.h, 0, 1, own + 4 * (n - 1), n) == INVALID_ARG
    h = ctypes.c_void_p()
    assert L.vx_grid_morph(g.h, 4, 1, ctypes.byref(h)) == INVALID_ARG and not h.value
    assert L.vx_grid_morph(g.h, 0, 0xFFFFFFFF, ctypes.byref(h)) == INVALID_ARG and not h.value
    assert L.vx_grid_seal(g.h, 0xFFFFFFFF, ctypes.byref(h)) == INVALID_ARG and not h.value
    assert L.vx_grid_morph(g.h, 0, 1, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert (host == 0x12345678).all() and (dev.cpu() == 0x1234567).all() and np.array_equal(g.bitmask(), w0)
    # a grid of 0 cells: VX_OK, nothing written
    z = gpu.Grid.create(gpu.GRID_BOOL, 0, 3, 3, F(0.5))
    assert L.vx_grid_morph_mask(z.h, 0, 1, host.ctypes.data, 0) == 0 and L.vx_grid_morph_device(z.h, 3, 100, dev.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert (host == 0x12345678).all() and (dev.cpu() == 0x1234567).all()
    assert z.dilate(radius=1).describe()["occupied"] == 0
    with pytest.raises(ValueError):
        g.dilate()
    with pytest.raises(ValueError):
        g.morph_mask_device(0, 1, out=torch.empty(n - 1, dtype=torch.int32, device="cuda") if n > 1 else torch.empty(1, dtype=torch.float32, device="cuda"))


def test_padded_domain_over_the_axis_limit(gpu):
    import torch
    X = 1 << 21
    g = gpu.Grid.create(gpu.GRID_BOOL, X, 1, 1, F(0.01))
    g.set_voxel(5, 0, 0)
    L = gpu.lib()
    n = g.describe()["num_words"]
    dev = torch.full((n,), 0x1234567, dtype=torch.int32, device="cuda")
    gpu.profile_enable(True)
    gpu.profile_reset()
    assert L.vx_grid_morph_device(g.h, gpu.MORPH_CLOSE, 1, dev.data_ptr(), n) == CAPACITY
    h = ctypes.c_void_p()
    assert L.vx_grid_seal(g.h, 0, ctypes.byref(h)) == CAPACITY and not h.value
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert not any("k_morph" in x or "k_dist" in x for x in names), names
    torch.cuda.synchronize()
    assert (dev.cpu() == 0x1234567).all()
    # the same grid takes the operations that do not pad; CLOSE at r2 = 0 pads by nothing
    want = np.zeros((1, 1, X), bool)
    want[0, 0, 4:7] = True
    assert np.array_equal(g.morph_mask(gpu.MORPH_DILATE, 1), solid_ref.pack(want))
    assert np.array_equal(g.morph_mask(gpu.MORPH_CLOSE, 0), g.bitmask())


# ---- the default path ---------------------------------------------------------------------------------------------------------------
def test_default_paths_queue_no_morph_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    rays = vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1)
    g.trace(rays)
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert names and not any("k_morph" in n for n in names), names


# ---- C++ facade and CLI -----------------------------------------------------------------------------------------------------------
def holed_obj(tmp_path):
    v, t = vx_scenes.holed_box(0.6)
    obj = tmp_path / "holed.obj"
    vx_scenes.write_obj(str(obj), v, t)
    return str(obj)


def test_facade_matches_reference(gpu, tmp_path):
    import build as vxbuild
    exe = str(tmp_path / "morph_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "morph_facade.cpp"), "-o", exe, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    obj = holed_obj(tmp_path)
    r = subprocess.run([exe, obj, "0.1", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(obj), F(0.1), gpu.GRID_BOOL)
    m = solid_ref.unpack(g.bitmask(), g.describe()["dim"])
    want = [int(x.sum()) for x in (m, mr.dilate_fast(m, 5, c=True), mr.erode_fast(m, 5, c=True), mr.open_fast(m, 5, c=True), mr.close_fast(m, 5, c=True),
                                   mr.seal_fast(m, 5, c=True))]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("bool", "aabbstruct", "vec")]
    assert [ln[0] for ln in lines] == ["bool", "aabbstruct", "vec"], r.stdout
    for ln in lines:
        assert [int(x) for x in ln[1:7]] == want, (ln, want)
        assert int(ln[7]) == want[5]


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_cli_seal_surface_is_closed(gpu, tmp_path):
    obj = holed_obj(tmp_path)
    out = tmp_path / "out.obj"
    r = run_cli([obj, "0.1", "--solid", "--seal", "2.3", "--surface", str(out)])
    assert r.returncode == 0, r.stdout + r.stderr
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(obj), F(0.1), gpu.GRID_BOOL, solid=True)
    m = solid_ref.unpack(g.bitmask(), g.describe()["dim"])
    want = mr.seal_fast(m, 5, c=True)
    mm = re.search(r"morph: seal r2=5 occupied (\d+) -> (\d+)", r.stdout)
    assert mm and (int(mm.group(1)), int(mm.group(2))) == (int(m.sum()), int(want.sum())), r.stdout
    faces = []
    for ln in out.read_text().splitlines():
        if ln.startswith("f "):
            faces.append([int(tok.split("/")[0]) for tok in ln.split()[1:]])
    assert faces
    edges = {}
    for f in faces:
        for a, b in zip(f, f[1:] + f[:1]):
            k = (min(a, b), max(a, b))
            edges[k] = edges.get(k, 0) + 1
    assert all(c % 2 == 0 for c in edges.values()), "the sealed surface has an open edge"
    sv, st_ = g.seal(radius=2.3).surface()
    assert len(faces) == len(st_)


@pytest.mark.parametrize("op,r2", [("dilate:1.5", 2), ("erode:1", 1), ("open:1", 1), ("close:2", 4)])
def test_cli_morph_dump(gpu, tmp_path, op, r2):
    obj = holed_obj(tmp_path)
    dump = tmp_path / "a.bin"
    r = run_cli([obj, "0.1", "--grid", "vec", "--morph", op, "--dump", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(obj), F(0.1), gpu.GRID_BOOL)
    code = {"dilate": 0, "erode": 1, "open": 2, "close": 3}[op.split(":")[0]]
    res = g._morph_grid(code, None, r2)
    assert dump.read_bytes() == res.aabbs().tobytes()
    assert re.search(r"morph: %s r2=%d occupied %d -> %d" % (op.split(":")[0], r2, g.describe()["occupied"], res.describe()["occupied"]), r.stdout), r.stdout


@pytest.mark.parametrize("extra", [["--grid", "octree", "--seal", "1"], ["--morph", "grow:1"], ["--morph", "dilate"], ["--morph", "dilate:x"], ["--seal", "-1"],
                                   ["--grid", "octree", "--morph", "open:1"], ["--materials", "--morph", "dilate:1"]])
def test_cli_refusals(gpu, tmp_path, extra):
    obj = holed_obj(tmp_path)
    r = run_cli([obj, "0.1"] + extra)
    assert r.returncode == 2 and r.stderr.strip() and "morph" not in r.stdout, (r.returncode, r.stdout, r.stderr)
