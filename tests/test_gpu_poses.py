"""GPU tests of the pose queries (vx_field_poses*): every output is compared bit for bit with the restatement (tests/poses_ref.py)
evaluated on the GPU's own sdf() of the same grid.  Sizes sit around the kernel's own: 64 points (a group of lanes per pose below, a
chunk of POSE_CHUNK points per workgroup above), POSE_CHUNK, and POSE_TILE poses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import field_cases as fc
import field_ref as fr
import poses_cases as pc
import poses_ref as pr
import vx_scenes
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG, CAPACITY = 1, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
NAMES = ("clearance", "point", "count", "position", "gradient")
PATTERN = 0xA5
CHUNK, TILE = 256, 32
POINT_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2 * CHUNK + 1]
POSE_COUNTS = [1, TILE - 1, TILE, TILE + 1, 1000]
GRIDS = {"1x1x1": ((1, 1, 1), 1.0), "2x1x3": ((2, 1, 3), 0.5), "5x4x3": ((5, 4, 3), 0.5), "40x36x31": ((40, 36, 31), None)}


def masked_grid(gpu, cells, vs):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, Z, vs, fc.ORG)
    write_mask(g, dr.pack(cells))
    g.refresh()
    return g


def case_cells(dims, density):
    if density is None:
        return fc.prototype_mask(dims)
    X, Y, Z = dims
    m = np.random.default_rng(X * 7 + Y * 3 + Z + int(density * 1e4)).random((Z, Y, X)) < density
    if 0.0 < density < 1.0 and m.size > 1:
        m.flat[0], m.flat[-1] = True, False
    return m


def geometry(g):
    d = g.describe()
    return g.sdf(), tuple(float(x) for x in d["origin"]), F(d["voxel_size"]), d["dim"]


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d entries differ" % (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def check_poses(f, ref, pts, xf, radii, margin, what="", n=None):
    """the query on the first n poses against the first n entries of a reference over all of xf (a pose's answer depends on no other)"""
    n = len(xf) if n is None else n
    got = f.poses(pts, xf[:n], radii=radii, margin=margin, want=NAMES)
    assert list(got) == list(NAMES)
    for name, r in zip(NAMES, ref):
        same_bits(got[name], r[:n], "%s %s (%d points, %d poses)" % (what, name, len(pts), n))
    return got


@pytest.fixture(scope="module")
def fields(gpu):
    """name -> grid, field, the GPU's own sdf(), origin, vs, dims, and 1000 poses in the box grown by 2 cells"""
    out = {}
    for name, (dims, density) in GRIDS.items():
        g = masked_grid(gpu, case_cells(dims, density), fc.VS_ODD)
        S, org, vs, d = geometry(g)
        assert tuple(d) == dims
        out[name] = dict(g=g, f=g.field(), S=S, org=org, vs=vs, dims=dims, xf=pc.transforms(dims, org, vs, 1000, 22))
    return out


@pytest.fixture(scope="module")
def proto(fields):
    """the main random case: the ball, plate and noise at 40 x 36 x 31, vs 0.37; 300 points in a ball of 2.5 cells with radii up to 1.5
    cells; 1000 random rotations translated inside the box grown by 2 cells; its restatement at margin 0"""
    c = dict(fields["40x36x31"])
    c["pts"], c["radii"] = pc.body(300, c["vs"], 21)
    c["ref"] = pr.poses(c["S"], c["org"], c["vs"], c["pts"], c["xf"], c["radii"], 0.0)
    return c


def test_main_case_is_not_one_sided_and_matches(gpu, proto):
    c, point, count, pos, grad = proto["ref"]
    print("colliding %.1f %%, %d distinct points" % (100.0 * (count > 0).mean(), len(np.unique(point))))
    assert (count > 0).mean() >= 0.2
    assert (count == 0).mean() >= 0.2
    assert len(np.unique(point)) >= 50
    check_poses(proto["f"], proto["ref"], proto["pts"], proto["xf"], proto["radii"], 0.0)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("P", POINT_COUNTS)
def test_point_and_pose_counts(gpu, fields, grid, P):
    c = fields[grid]
    pts, radii = pc.body(P, c["vs"], 100 + P)
    margin = float(F(0.25) * c["vs"])
    ref = pr.poses(c["S"], c["org"], c["vs"], pts, c["xf"], radii, margin)
    if P == 0:
        assert (ref[1] == pr.NO_POINT).all() and np.isposinf(ref[0]).all() and not ref[2].any()
    for N in POSE_COUNTS:
        check_poses(c["f"], ref, pts, c["xf"], radii, margin, grid, n=N)
    check_poses(c["f"], pr.poses(c["S"], c["org"], c["vs"], pts, c["xf"][:TILE + 1], None, margin), pts, c["xf"][:TILE + 1], None, margin, grid + " no radii")


@pytest.mark.parametrize("P,N", [(1, 2100), (2, 1100), (3, 600), (5, 300), (9, 200), (17, 130), (33, 70), (64, 40)])
def test_every_group_width_over_several_workgroups(gpu, proto, P, N):
    """P <= 64: a group of 2^k >= P lanes per pose and 8 * 256 / 2^k poses per workgroup; N lies past that in every case"""
    c = proto
    xf = pc.transforms(c["dims"], c["org"], c["vs"], N, 31)
    pts, radii = c["pts"][:P], c["radii"][:P]
    ref = pr.poses(c["S"], c["org"], c["vs"], pts, xf, radii, 0.0)
    assert (ref[2] > 0).any() and (ref[2] == 0).any()
    check_poses(c["f"], ref, pts, xf, radii, 0.0)


@pytest.mark.parametrize("density", [0.0, 1.0])
@pytest.mark.parametrize("P", [20, 300])
def test_empty_and_full_fields(gpu, density, P):
    dims = (5, 4, 3)
    g = masked_grid(gpu, case_cells(dims, density), fc.VS_ODD)
    S, org, vs, d = geometry(g)
    f = g.field()
    assert f.describe()["state"] == (gpu.FIELD_EMPTY if density == 0.0 else gpu.FIELD_FULL)
    pts, radii = pc.body(P, vs, 5)
    xf = pc.transforms(dims, org, vs, 70, 6)
    for r in (None, radii):
        ref = pr.poses(S, org, vs, pts, xf, r, 0.0)
        assert (ref[1] == 0).all() and (np.isposinf(ref[0]) if density == 0.0 else np.isneginf(ref[0])).all()   # +-inf takes part
        assert (ref[2] == (0 if density == 0.0 else P)).all() and not ref[4].any()
        check_poses(f, ref, pts, xf, r, 0.0)
    for what, p, r, m in pc.nonfinite_variants(pts, radii, xf):
        check_poses(f, pr.poses(S, org, vs, p, m, r, 0.0), p, m, r, 0.0, what)
    f.free()
    g.free()


@pytest.mark.parametrize("P", [20, 70, 300])
def test_non_finite_entries(gpu, proto, P):
    c = proto
    pts, radii, xf = c["pts"][:P], c["radii"][:P], c["xf"][:100]
    seen = set()
    for what, p, r, m in pc.nonfinite_variants(pts, radii, xf):
        ref = pr.poses(c["S"], c["org"], c["vs"], p, m, r, 0.0)
        check_poses(c["f"], ref, p, m, r, 0.0, what)
        none = ref[1] == pr.NO_POINT
        if what == "transform entries":
            assert none[3:7].all() and not none[7:].any()   # a pose whose every point is skipped
        if what == "radii":
            assert np.isneginf(ref[0]).all() and (ref[1] == P // 3).all()
        seen.add(what)
    assert seen == {"points", "radii", "transform entries", "overflowing transforms"}
    # every point skipped on every pose
    ref = pr.poses(c["S"], c["org"], c["vs"], np.full_like(pts, np.nan), xf, radii, 0.0)
    assert (ref[1] == pr.NO_POINT).all()
    check_poses(c["f"], ref, np.full_like(pts, np.nan), xf, radii, 0.0, "all skipped")


@pytest.mark.parametrize("margin", [float("inf"), float("-inf"), -0.2, 0.3])
def test_margins(gpu, proto, margin):
    c = proto
    for P in (20, 300):
        pts, radii = c["pts"][:P].copy(), c["radii"][:P].copy()
        pts[1, 0] = np.nan                     # a skipped point is counted under no margin
        radii[2] = np.inf                      # g = -inf: counted under every margin
        ref = pr.poses(c["S"], c["org"], c["vs"], pts, c["xf"][:200], radii, margin)
        if margin == float("inf"):
            assert (ref[2] == P - 1).all()
        if margin == float("-inf"):
            assert (ref[2] == 1).all()
        check_poses(c["f"], ref, pts, c["xf"][:200], radii, margin)


@pytest.mark.parametrize("P", [20, 300])
def test_each_output_alone(gpu, proto, P):
    c = proto
    pts, radii, xf = c["pts"][:P], c["radii"][:P], c["xf"][:100]
    ref = pr.poses(c["S"], c["org"], c["vs"], pts, xf, radii, 0.0)
    for name, r in zip(NAMES, ref):
        one = c["f"].poses(pts, xf, radii=radii, want=(name,))
        assert list(one) == [name]
        same_bits(one[name], r, name + " alone")
    assert list(c["f"].poses(pts, xf, radii=radii)) == ["clearance", "point", "count"]


def test_mesh_field_in_all_grid_kinds(gpu):
    v, t = vx_scenes.scene("rotcube")
    mesh = gpu.Mesh.from_arrays(v, t)
    first = None
    for kind in (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC):
        g = gpu.Grid.voxelize(mesh, F(0.09), kind)
        S, org, vs, dims = geometry(g)
        f = g.field()
        pts, radii = pc.body(90, vs, 8)
        xf = pc.transforms(dims, org, vs, 200, 9)
        ref = pr.poses(S, org, vs, pts, xf, radii, 0.0)
        got = check_poses(f, ref, pts, xf, radii, 0.0)
        if first is None:
            first = got
            assert (ref[2] > 0).any() and (ref[2] == 0).any()
        for k in NAMES:
            same_bits(got[k], first[k], "grid kinds")
        f.free()


# ---- handle behaviour ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [20, 300])
def test_device_variant_equals_host_variant(gpu, proto, P):
    import torch
    c = proto
    pts, radii, xf = c["pts"][:P], c["radii"][:P], c["xf"]
    N = len(xf)
    dp, dr_, dx = torch.from_numpy(pts).cuda(), torch.from_numpy(radii).cuda(), torch.from_numpy(xf).cuda()
    out = dict(clearance=torch.empty(N, dtype=torch.float32, device="cuda"), point=torch.empty(N, dtype=torch.int32, device="cuda"),
               count=torch.empty(N, dtype=torch.int32, device="cuda"), position=torch.empty((N, 3), dtype=torch.float32, device="cuda"),
               gradient=torch.empty((N, 3), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    c["f"].poses_device(dp.data_ptr(), P, dx.data_ptr(), N, radii_ptr=dr_.data_ptr(), margin=0.1, **{k: v.data_ptr() for k, v in out.items()})
    torch.cuda.synchronize()
    host = c["f"].poses(pts, xf, radii=radii, margin=0.1, want=NAMES)
    ref = pr.poses(c["S"], c["org"], c["vs"], pts, xf, radii, 0.1)
    for name, r in zip(NAMES, ref):
        d = out[name].cpu().numpy()
        same_bits(d.view(np.uint32) if d.dtype == np.int32 else d, host[name], name)
        same_bits(host[name], r, name + " against the restatement")
    # one output, no radii
    only = torch.empty(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c["f"].poses_device(dp.data_ptr(), P, dx.data_ptr(), N, count=only.data_ptr())
    torch.cuda.synchronize()
    same_bits(only.cpu().numpy().view(np.uint32), pr.poses(c["S"], c["org"], c["vs"], pts, xf, None, 0.0)[2], "count alone, device")
    with pytest.raises(ValueError):
        c["f"].poses_device(dp.data_ptr(), P, dx.data_ptr(), N, value=only.data_ptr())


def test_queries_after_update_and_after_the_grid_is_freed(gpu):
    dims = (33, 9, 7)
    a, b = case_cells(dims, 0.3), case_cells(dims, 0.01)
    g = masked_grid(gpu, a, fc.VS_ODD)
    f = g.field()
    pts, radii = pc.body(300, fc.VS_ODD, 3)
    xf = pc.transforms(dims, fc.ORG, fc.VS_ODD, 100, 4)
    S, org, vs, d = geometry(g)
    before = pr.poses(S, org, vs, pts, xf, radii, 0.0)
    check_poses(f, before, pts, xf, radii, 0.0, "before the update")
    write_mask(g, dr.pack(b))
    g.refresh()
    S, org, vs, d = geometry(g)
    n0 = gpu.device_allocations()
    f.update(g)
    ref = pr.poses(S, org, vs, pts, xf, radii, 0.0)
    check_poses(f, ref, pts, xf, radii, 0.0, "after the update")
    assert gpu.device_allocations() == n0
    assert (ref[2] > 0).any() and (ref[2] == 0).any() and (before[2] > 0).all()   # (the update changed the answers)
    g.free()
    junk = masked_grid(gpu, case_cells((64, 64, 64), 0.5), fc.VS_DYADIC)  # (takes the freed grid's blocks from the pool)
    junk.sdf()
    check_poses(f, ref, pts, xf, radii, 0.0, "after the grid is freed")
    check_poses(f, pr.poses(S, org, vs, pts[:20], xf, radii[:20], 0.0), pts[:20], xf, radii[:20], 0.0, "after the grid is freed")
    f.free()
    junk.free()


def test_repeated_queries_allocate_nothing_and_free_returns_every_block(gpu, proto):
    c = proto
    g = masked_grid(gpu, case_cells(c["dims"], None), fc.VS_ODD)
    g.sdf()
    live0 = gpu.device_live_blocks()
    f = g.field()
    live1 = gpu.device_live_blocks()
    assert live1 > live0
    f.poses(c["pts"], c["xf"], radii=c["radii"], want=NAMES)
    f.poses(c["pts"][:20], c["xf"], radii=c["radii"][:20], want=NAMES)
    assert gpu.device_live_blocks() > live1    # the staging blocks and the scratch stay on the handle
    n0 = gpu.device_allocations()
    a = f.poses(c["pts"], c["xf"], radii=c["radii"], want=NAMES)
    b = f.poses(c["pts"][:20], c["xf"], radii=c["radii"][:20], want=NAMES)
    f.sample(c["pts"][:20])
    assert gpu.device_allocations() == n0
    for name, r in zip(NAMES, c["ref"]):
        same_bits(a[name], r, name)
    same_bits(b["clearance"], pr.poses(c["S"], c["org"], c["vs"], c["pts"][:20], c["xf"], c["radii"][:20], 0.0)[0], "clearance")
    f.free()
    assert gpu.device_live_blocks() == live0
    g.free()


def test_poisoned_pool_blocks_change_nothing(gpu, proto):
    c = proto
    gpu.pool_poison(0xA5A5A5A5)
    try:
        g = masked_grid(gpu, case_cells(c["dims"], None), fc.VS_ODD)
        f = g.field()
        check_poses(f, c["ref"], c["pts"], c["xf"], c["radii"], 0.0, "poisoned")
        for P in (20, 70):
            check_poses(f, pr.poses(c["S"], c["org"], c["vs"], c["pts"][:P], c["xf"], c["radii"][:P], 0.0), c["pts"][:P], c["xf"], c["radii"][:P], 0.0, "poisoned")
        for name, r in zip(NAMES, c["ref"]):
            same_bits(f.poses(c["pts"], c["xf"], radii=c["radii"], want=(name,))[name], r, name + " alone, poisoned")
        f.free()
        g.free()
    finally:
        gpu.pool_poison(None)


def patterned(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, PATTERN, dtype=np.uint8).view(dtype)


def test_argument_checks_write_nothing(gpu, proto):
    L, f = gpu.lib(), proto["f"]
    P, N = 20, 40
    pts = np.ascontiguousarray(proto["pts"][:P])
    radii = np.ascontiguousarray(proto["radii"][:P])
    xf = np.ascontiguousarray(proto["xf"][:N])
    outs = dict(clearance=patterned(N, F), point=patterned(N, np.uint32), count=patterned(N, np.uint32), position=patterned(3 * N, F),
                gradient=patterned(3 * N, F))

    def untouched():
        return all((a.view(np.uint8) == PATTERN).all() for a in outs.values())

    def args(points=pts.ctypes.data, num_points=P, transforms=xf.ctypes.data, num_poses=N, margin=0.0, names=NAMES):
        a = gpu.FieldPoseArgs()
        a.points, a.num_points, a.radii, a.transforms, a.num_poses, a.margin = points, num_points, radii.ctypes.data, transforms, num_poses, margin
        for k in names:
            setattr(a, k, outs[k].ctypes.data)
        return a

    for fn in (L.vx_field_poses, L.vx_field_poses_device):
        assert fn(None, C.byref(args())) == INVALID_ARG
        assert fn(f.h, None) == INVALID_ARG
        assert fn(f.h, C.byref(args(transforms=None))) == INVALID_ARG
        assert fn(f.h, C.byref(args(points=None))) == INVALID_ARG
        assert fn(f.h, C.byref(args(names=()))) == INVALID_ARG
        assert fn(f.h, C.byref(args(margin=float("nan")))) == INVALID_ARG
        assert fn(f.h, C.byref(args(num_points=0xFFFFFFFF))) == CAPACITY
        assert fn(f.h, C.byref(args(num_points=1 << 40))) == CAPACITY
        assert fn(f.h, C.byref(args(num_poses=0))) == 0
        assert fn(f.h, C.byref(args(transforms=None, num_poses=0))) == 0
        assert untouched()
    # the host variant with the same arguments and nothing wrong writes every output; zero points with NULL points is "none" on every pose
    assert L.vx_field_poses(f.h, C.byref(args(margin=float("inf")))) == 0
    ref = pr.poses(proto["S"], proto["org"], proto["vs"], pts, xf, radii, float("inf"))
    for name, r in zip(NAMES, ref):
        same_bits(outs[name].reshape(r.shape), r, name)
    assert L.vx_field_poses(f.h, C.byref(args(points=None, num_points=0))) == 0
    assert (outs["point"] == pr.NO_POINT).all() and np.isposinf(outs["clearance"]).all() and not outs["count"].any()
    assert not outs["position"].any() and not outs["gradient"].any()


def test_default_paths_queue_no_pose_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    g.trace(vx_scenes.random_rays(1000, np.array([-1.5] * 3, np.float32), np.array([1.5] * 3, np.float32), seed=1))
    f = g.field()
    f.sample(np.zeros((4, 3), dtype=F))
    f.sphere_trace(np.ones((4, 6), dtype=F))
    names = list(gpu.profile_read())
    assert names and not any("k_field_poses" in n for n in names), names
    gpu.profile_reset()
    xf = np.tile(pc.IDENTITY, (3, 1))
    f.poses(np.zeros((4, 3), dtype=F), xf)
    names = list(gpu.profile_read())
    assert "k_field_poses_narrow" in names and "k_field_poses_finish" in names and "k_field_poses" not in names, names
    gpu.profile_reset()
    f.poses(np.zeros((65, 3), dtype=F), xf)
    names = list(gpu.profile_read())
    gpu.profile_enable(False)
    assert "k_field_poses" in names and "k_field_poses_finish" in names and "k_field_poses_narrow" not in names, names


# ---- C++ facade and CLI -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rotcube(gpu, tmp_path_factory):
    """the rotated cube at 0.09 as an OBJ file, its Python field, a body of 90 spheres and 300 poses (some with non-finite entries)"""
    d = tmp_path_factory.mktemp("poses_cli")
    v, t = vx_scenes.scene("rotcube")
    obj = d / "r.obj"
    vx_scenes.write_obj(str(obj), v, t)
    g = gpu.Grid.voxelize(gpu.Mesh.load_obj(str(obj)), F(0.09), gpu.GRID_BOOL)
    S, org, vs, dims = geometry(g)
    pts, radii = pc.body(90, vs, 8)
    xf = pc.transforms(dims, org, vs, 300, 9)
    xf[5, 3], xf[6, :], xf[7, 0] = np.nan, np.inf, -np.inf
    return dict(dir=d, obj=str(obj), g=g, f=g.field(), org=org, vs=vs, dims=dims, pts=pts, radii=radii, xf=xf)


def test_facade_matches_python(gpu, rotcube):
    import build as vxbuild
    c = rotcube
    exe = str(c["dir"] / "poses_facade")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", vxbuild.CPP,
                           "-I", os.path.join(vxbuild.ROOT, "include"), "-isystem", os.path.join(vxbuild.ROCM, "include"),
                           os.path.join(ROOT, "tests", "poses_facade.cpp"), "-o", exe, "-L", vxbuild.HERE, "-lvoxhip",
                           "-L", os.path.join(vxbuild.ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + vxbuild.HERE, "-lpthread"])
    pf, rf, xf, out = c["dir"] / "p.f32", c["dir"] / "r.f32", c["dir"] / "x.f32", c["dir"] / "o.bin"
    pf.write_bytes(c["pts"].tobytes())
    xf.write_bytes(c["xf"].tobytes())
    margin = float(F(0.02))
    for radii in (c["radii"], None):
        rf.write_bytes(radii.tobytes() if radii is not None else b"")
        r = subprocess.run([exe, c["obj"], repr(float(F(0.09))), str(pf), str(rf), str(xf), repr(margin), str(out)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        a = c["f"].poses(c["pts"], c["xf"], radii=radii, margin=margin, want=NAMES)
        assert (a["count"] > 0).any() and (a["count"] == 0).any() and (a["point"] == pr.NO_POINT).any()
        part = b"".join(a[k].tobytes() for k in NAMES)
        raw = out.read_bytes()
        assert len(raw) == 3 * len(part)
        for k in range(3):
            assert raw[k * len(part):(k + 1) * len(part)] == part, "flavour %d" % k


def run_cli(args):
    return subprocess.run([os.path.join(PKG, "voxilizer")] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)


@pytest.mark.parametrize("grid", ["bool", "vec"])
def test_cli_poses(gpu, rotcube, grid):
    c = rotcube
    body, poses, pout = c["dir"] / "body.txt", c["dir"] / "poses.txt", c["dir"] / ("poses_%s.txt" % grid)
    # (half of the lines carry a radius, the rest have radius 0)
    radii = np.where(np.arange(len(c["pts"])) % 2 == 0, c["radii"], F(0)).astype(F)
    body.write_text("".join(("%.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], r)) if k % 2 == 0 else ("%.9g %.9g %.9g\n" % tuple(p))
                            for k, (p, r) in enumerate(zip(c["pts"], radii))))
    poses.write_text("".join(" ".join("%.9g" % x for x in m) + "\n" for m in c["xf"]))
    margin = F(0.02)
    r = run_cli([c["obj"], "0.09", "--grid", grid, "--poses", str(poses), "--body", str(body), "--pose-margin", "%.9g" % margin, "--pose-out", str(pout)])
    assert r.returncode == 0, r.stdout
    rows = [ln.split() for ln in pout.read_text().splitlines()]
    assert len(rows) == len(c["xf"]) and all(len(x) == 9 for x in rows)
    a = c["f"].poses(c["pts"], c["xf"], radii=radii, margin=float(margin), want=NAMES)
    same_bits(np.array([float(x[0]) for x in rows], dtype=F), a["clearance"], "clearance")   # (no NaN among the outputs)
    same_bits(np.array([int(x[1]) for x in rows], dtype=np.uint32), a["point"], "point")
    same_bits(np.array([int(x[2]) for x in rows], dtype=np.uint32), a["count"], "count")
    same_bits(np.array([[float(y) for y in x[3:6]] for x in rows], dtype=F), a["position"], "position")
    same_bits(np.array([[float(y) for y in x[6:9]] for x in rows], dtype=F), a["gradient"], "gradient")
    colliding = int((a["count"] > 0).sum())
    assert 0 < colliding < len(rows) and (a["point"] == pr.NO_POINT).any()
    assert "[voxhip] poses: %d poses of %d points" % (len(rows), len(c["pts"])) in r.stdout and "%d colliding" % colliding in r.stdout


@pytest.mark.parametrize("args", [["--poses", "p.txt", "--body", "b.txt", "--grid", "octree"], ["--poses", "p.txt", "--body", "b.txt", "--bench", "2"],
                                  ["--poses", "p.txt", "--body", "b.txt", "--gpus", "2"], ["--poses", "p.txt"], ["--body", "b.txt"],
                                  ["--pose-margin", "1"], ["--pose-out", "o.txt"], ["--poses", "p.txt", "--body", "b.txt", "--pose-margin", "nan"]])
def test_cli_refusals(gpu, rotcube, args):
    r = run_cli([rotcube["obj"], "0.09"] + args)
    assert r.returncode == 2 and ("--poses" in r.stdout or "--pose-margin" in r.stdout), r.stdout
