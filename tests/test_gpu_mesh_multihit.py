"""GPU tests of the multi-hit ray queries on triangles (vx_bvh_trace_multi*, vx_tlas_trace_multi*; Bvh.trace_multi, Tlas.trace_multi): the
ordered hit lists, their prims, instances and barycentrics, and the hit counts are compared whole, bit for bit (floats through their
uint32 view), with the numpy brute force of tests/mesh_multihit_ref.py on the inputs of tests/mesh_multihit_cases.py."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_multihit_cases as mc
import mesh_multihit_ref as mm
import oracle
import vx_scenes

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG = 1
# every compiled list size KC = 4, 8, 16, 32 exactly full (K = KC) and at its smallest K (5, 9, 17)
KS = (1, 4, 5, 8, 9, 16, 17, 32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
ALL = ("t", "prim", "bary", "count")
ALL_TLAS = ("t", "instance", "prim", "bary", "count")


def same(got, ref, what=""):
    """whole arrays, floats through their bits"""
    for f in got:
        g, r = got[f], ref[f]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, f, g.shape, r.shape)
        if g.dtype == F:
            g, r = g.view(np.uint32), r.view(np.uint32)
        bad = np.flatnonzero((g != r).reshape(len(g), -1).any(axis=1))
        assert not len(bad), "%s %s: %d rays differ, first %d: %r want %r" % (what, f, len(bad), bad[0], got[f][bad[0]], ref[f][bad[0]])


@functools.lru_cache(maxsize=None)
def bvhs(name):
    import voxhip as gpu
    c = mc.bvh_case(name)
    mesh = gpu.Mesh.from_arrays(c.v, c.t)
    return tuple(mesh.bvh(max_leaf=m) for m in c.max_leaf)


@functools.lru_cache(maxsize=None)
def tlas():
    import voxhip as gpu
    c = mc.tlas_case()
    bl = [gpu.Mesh.from_arrays(v, t).bvh() for v, t in c.meshes]
    return gpu.Tlas(bl, c.inst)


# ---- one BVH ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", mc.BVH_CASES)
def test_bvh_lists_and_counts(gpu, name, k):
    c = mc.bvh_case(name)
    ref = mm.select(c.hits, k)
    for m, b in zip(c.max_leaf, bvhs(name)):
        what = "%s max_leaf=%d K=%d" % (name, m, k)
        got = b.trace_multi(c.rays, max_hits=k, want=ALL)
        same(got, ref, what)
        pad = np.arange(k)[None, :] >= np.minimum(ref["count"], k)[:, None]
        assert (got["t"][pad] == F(-1)).all() and (got["prim"][pad] == 0xFFFFFFFF).all() and not got["bary"][pad].any()
        # without the count the ray may stop early: the same lists; and the count alone
        same(b.trace_multi(c.rays, max_hits=k, want=("t", "prim", "bary")), ref, what + ", no count")
        same(b.trace_multi(c.rays, max_hits=k, want=("count",)), ref, what + ", count only")
        # slot 0 is the first-hit query's answer
        one = b.trace_ex(c.rays, want=("t", "prim", "bary"))
        assert np.array_equal(got["t"][:, 0].view(np.uint32), one["t"].view(np.uint32)) and np.array_equal(got["prim"][:, 0], one["prim"])
        assert np.array_equal(got["bary"][:, 0].view(np.uint32), one["bary"].view(np.uint32))


def test_bvh_side_listed_triangles_count_once(gpu):
    """`adversarial`: rays that accept a side-listed triangle (tests/test_mesh_multihit_cpu.py asserts there are some) count it once"""
    c = mc.bvh_case("adversarial")
    b = bvhs("adversarial")[0]
    assert b.num_ill_conditioned == int(mc.side_listed(c.v, c.t).sum()) > 50
    ill_rays = np.unique(c.hits.ray[mc.side_listed(c.v, c.t)[c.hits.prim]])
    assert len(ill_rays) >= 10
    got = b.trace_multi(c.rays, max_hits=1, want=("count",))["count"]
    assert np.array_equal(got[ill_rays], mm.select(c.hits, 1)["count"][ill_rays])
    assert np.array_equal(b.leaf_triangles()[np.argsort(b.leaf_triangles())], np.arange(len(c.t)))   # the marker changed no output of the build


@pytest.mark.parametrize("name", ["layers", "floor", "blob"])
def test_bvh_windows(gpu, name):
    """tmin / tmax that cut the lists in the middle, bounds that ARE hit times (inclusive), and a tmax per ray"""
    c = mc.bvh_case(name)
    b = bvhs(name)[-1]
    pos = np.sort(c.hits.t)
    lo, hi = float(pos[int(0.35 * len(pos))]), float(pos[int(0.65 * len(pos))])
    ref = mm.select(mm.all_hits(c.v, c.t, c.rays, tmin=lo, tmax=hi), 8)
    assert 0 < ref["count"].sum() < len(pos)
    same(b.trace_multi(c.rays, max_hits=8, tmin=lo, tmax=hi, want=ALL), ref, "window")
    t4 = mm.select(c.hits, 4)["t"]
    tpr = np.where(t4[:, 2] > 0, t4[:, 2], F(10000.0)).astype(F)     # the third hit's own t: the list ends with it and its ties
    ref = mm.select(mm.all_hits(c.v, c.t, c.rays, tmax_per_ray=tpr), 8)
    assert (ref["count"] >= 3).any()
    same(b.trace_multi(c.rays, max_hits=8, tmax_per_ray=tpr, want=ALL), ref, "tmax_per_ray")
    same(b.trace_multi(c.rays, max_hits=2, tmax_per_ray=tpr, want=("t", "prim")), mm.select(mm.all_hits(c.v, c.t, c.rays, tmax_per_ray=tpr), 2), "tmax_per_ray, no count")


@pytest.mark.parametrize("k", [5, 16, 32])
def test_bvh_paging_with_the_cursor(gpu, k):
    """`layers`: pages chained through `after` until every ray is exhausted (K = 32: three pages of its 80 hits, K = 16: five; K = 5 ends pages inside
    runs of equal t) reassemble the whole list and count down the total"""
    c = mc.bvh_case("layers")
    b = bvhs("layers")[0]
    total = mm.select(c.hits, 1)["count"]
    npages = -(-int(total.max()) // k)
    assert npages == {5: 16, 16: 5, 32: 3}[k]
    whole = mm.select(c.hits, k * npages)
    n = len(c.rays)
    cur = (np.full(n, F(-1), F), np.full(n, 12345, np.uint32))   # (-1, anything) = no cursor
    pages = []
    for page in range(npages + 1):
        got = b.trace_multi(c.rays, max_hits=k, after=cur, want=ALL)
        same(got, mm.select(c.hits, k, after=cur), "page %d" % page)
        assert np.array_equal(got["count"], np.maximum(total.astype(np.int64) - k * page, 0))
        pages.append(got)
        last = cur
        cur = mm.cursor_of(got, cur)
    assert not pages[-1]["count"].any()
    for f in ("t", "prim", "bary"):
        assert np.array_equal(np.concatenate([p[f] for p in pages[:-1]], axis=1), whole[f])
    # the early-out path under a cursor
    same(b.trace_multi(c.rays, max_hits=2, after=last, want=("t", "prim")), mm.select(c.hits, 2, after=last), "last page, no count")


def test_bvh_camera_rays(gpu):
    """rays generated in the kernel: the host's restatement of them by ray buffer gives the same lists but for the few pixels whose
    generated direction differs in the last bit (the rule of test_bvh_trace_camera)"""
    c = mc.bvh_case("floor")
    b = bvhs("floor")[0]
    vi, pi = vx_scenes.camera_matrices(aspect=48.0 / 32.0)
    W, H = 48, 32
    cam = b.trace_multi(camera=(vi, pi, W, H), max_hits=4, want=ALL)
    rays = oracle.primary_rays(vi, pi, W, H)
    ref = mm.select(mm.all_hits(c.v, c.t, rays), 4)
    same(b.trace_multi(rays, max_hits=4, want=ALL), ref, "restated camera rays")
    assert (ref["count"] >= 3).mean() > 0.02 and (ref["count"] == 0).any()
    ok = (cam["t"] == ref["t"]).all(axis=1) & (cam["prim"] == ref["prim"]).all(axis=1) & (cam["count"] == ref["count"])
    assert ok.mean() > 0.99


# ---- a TLAS -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_tlas_lists_and_counts(gpu, k):
    c = mc.tlas_case()
    tl = tlas()
    ref = mm.select(c.hits, k)
    got = tl.trace_multi(c.rays, max_hits=k, want=ALL_TLAS)
    same(got, ref, "K=%d" % k)
    pad = got["t"] < 0
    assert (got["instance"][pad] == 0xFFFFFFFF).all() and (got["prim"][pad] == 0xFFFFFFFF).all() and not got["bary"][pad].any()
    same(tl.trace_multi(c.rays, max_hits=k, want=("t", "instance", "prim", "bary")), ref, "K=%d, no count" % k)
    same(tl.trace_multi(c.rays, max_hits=k, want=("count",)), ref, "K=%d, count only" % k)
    one = tl.trace_ex(c.rays, want=("t", "instance", "prim", "bary"))
    for f in ("t", "instance", "prim", "bary"):
        assert np.array_equal(np.ascontiguousarray(got[f][:, 0]).view(np.uint32), one[f].view(np.uint32)), f


def test_tlas_windows(gpu):
    c = mc.tlas_case()
    tl = tlas()
    pos = np.sort(c.hits.t)
    lo, hi = float(pos[int(0.35 * len(pos))]), float(pos[int(0.65 * len(pos))])
    same(tl.trace_multi(c.rays, max_hits=8, tmin=lo, tmax=hi, want=ALL_TLAS), mm.select(mm.all_hits_tlas(c.meshes, c.inst, c.rays, tmin=lo, tmax=hi), 8), "window")
    t4 = mm.select(c.hits, 4)["t"]
    tpr = np.where(t4[:, 1] > 0, t4[:, 1], F(10000.0)).astype(F)     # the second hit's own t: on the twin instances that is the first hit's tie
    ref = mm.select(mm.all_hits_tlas(c.meshes, c.inst, c.rays, tmax_per_ray=tpr), 8)
    same(tl.trace_multi(c.rays, max_hits=8, tmax_per_ray=tpr, want=ALL_TLAS), ref, "tmax_per_ray")
    same(tl.trace_multi(c.rays, max_hits=1, tmax_per_ray=tpr, want=("t", "instance", "prim")), mm.select(mm.all_hits_tlas(c.meshes, c.inst, c.rays, tmax_per_ray=tpr), 1), "no count")


def test_tlas_paging_with_the_cursor(gpu):
    """K = 3 on the twin instances: pages end between two hits of one t, where the cursor's instance part decides"""
    c = mc.tlas_case()
    tl = tlas()
    k = 3
    total = mm.select(c.hits, 1)["count"]
    npages = -(-int(total.max()) // k)
    whole = mm.select(c.hits, k * npages)
    cur, pages = None, []
    for page in range(npages + 1):
        got = tl.trace_multi(c.rays, max_hits=k, after=cur, want=ALL_TLAS)
        same(got, mm.select(c.hits, k, after=cur), "page %d" % page)
        pages.append(got)
        cur = mm.cursor_of(got, cur, tlas=True)
    assert not pages[-1]["count"].any()
    for f in ("t", "instance", "prim", "bary"):
        assert np.array_equal(np.concatenate([p[f] for p in pages[:-1]], axis=1), whole[f])


def test_tlas_camera_rays(gpu):
    c = mc.tlas_case()
    tl = tlas()
    vi, pi = vx_scenes.camera_matrices(eye=(9.0, 4.0, -7.0), ctr=(0.5, 0.0, 0.3), aspect=48.0 / 32.0)
    W, H = 48, 32
    rays = oracle.primary_rays(vi, pi, W, H)
    ref = mm.select(mm.all_hits_tlas(c.meshes, c.inst, rays), 4)
    assert (ref["count"] >= 2).mean() > 0.02
    same(tl.trace_multi(rays, max_hits=4, want=ALL_TLAS), ref, "restated camera rays")
    cam = tl.trace_multi(camera=(vi, pi, W, H), max_hits=4, want=ALL_TLAS)
    ok = (cam["t"] == ref["t"]).all(axis=1) & (cam["instance"] == ref["instance"]).all(axis=1) & (cam["count"] == ref["count"])
    assert ok.mean() > 0.99


# ---- the device variants, side effects, errors ------------------------------------------------------------------------------------------
def test_device_variants_allocate_once(gpu):
    import torch

    def dev(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device="cuda")
    k = 8
    for tl_, handle, case in ((False, bvhs("blob")[0], mc.bvh_case("blob")), (True, tlas(), mc.tlas_case())):
        n = len(case.rays)
        d_rays = torch.from_numpy(case.rays).cuda()
        d_t, d_p, d_i, d_b, d_c = dev((n, k), torch.float32), dev((n, k), torch.int32), dev((n, k), torch.int32), dev((n, k, 2), torch.float32), dev(n, torch.int32)
        torch.cuda.synchronize()
        extra = dict(instance_ptr=d_i.data_ptr()) if tl_ else {}

        def run():
            handle.trace_multi_device(d_rays.data_ptr(), n, k, d_t.data_ptr(), d_p.data_ptr(), d_c.data_ptr(), bary_ptr=d_b.data_ptr(), **extra)
        run()
        before = gpu.device_allocations()
        run()
        run()
        assert gpu.device_allocations() == before
        torch.cuda.synchronize()
        got = {"t": d_t.cpu().numpy(), "prim": d_p.cpu().numpy().view(np.uint32), "bary": d_b.cpu().numpy(), "count": d_c.cpu().numpy().view(np.uint32)}
        if tl_:
            got["instance"] = d_i.cpu().numpy().view(np.uint32)
        same(got, mm.select(case.hits, k), "device, tlas=%s" % tl_)
        # camera rays on the device variant: what the host variant gives
        vi, pi = vx_scenes.camera_matrices(eye=(9.0, 4.0, -7.0), ctr=(0.5, 0.0, 0.3), aspect=1.0)
        W = H = 24
        d_t2, d_c2 = dev((W * H, k), torch.float32), dev(W * H, torch.int32)
        handle.trace_multi_device(None, 0, k, d_t2.data_ptr(), None, d_c2.data_ptr(), camera=(vi, pi, W, H))
        torch.cuda.synchronize()
        host = handle.trace_multi(camera=(vi, pi, W, H), max_hits=k, want=("t", "count"))
        assert (host["count"] > 0).any()
        assert np.array_equal(d_t2.cpu().numpy().view(np.uint32), host["t"].view(np.uint32))
        assert np.array_equal(d_c2.cpu().numpy().view(np.uint32), host["count"])


def test_empty_structures_and_zero_rays(gpu):
    rays = mc.bvh_case("cube").rays
    empty = gpu.Mesh.from_arrays(np.zeros((3, 3), F), np.zeros((0, 3), np.int32)).bvh()
    got = empty.trace_multi(rays, max_hits=3, want=ALL)
    assert (got["t"] == F(-1)).all() and (got["prim"] == 0xFFFFFFFF).all() and not got["bary"].any() and not got["count"].any()
    cube = bvhs("cube")[0]
    for tl in (gpu.Tlas([cube], gpu.instances(np.zeros((0, 12), F))),                                # zero instances
               gpu.Tlas([cube, empty], gpu.instances([np.eye(3, 4).reshape(12)] * 2, blas=[0, 1], mask=[0, 0xFF]))):  # none active
        got = tl.trace_multi(rays, max_hits=3, want=ALL_TLAS)
        assert (got["t"] == F(-1)).all() and (got["instance"] == 0xFFFFFFFF).all() and (got["prim"] == 0xFFFFFFFF).all()
        assert not got["bary"].any() and not got["count"].any()
    L = gpu.lib()
    a, b = gpu.BvhMultiHitArgs(), gpu.TlasMultiHitArgs()
    a.m.max_hits = b.m.max_hits = 4
    assert L.vx_bvh_trace_multi(cube.h, C.byref(a)) == 0 and L.vx_bvh_trace_multi_device(cube.h, C.byref(a)) == 0
    assert L.vx_tlas_trace_multi(tlas().h, C.byref(b)) == 0 and L.vx_tlas_trace_multi_device(tlas().h, C.byref(b)) == 0


def test_argument_errors_write_nothing(gpu):
    c = mc.bvh_case("cube")
    L = gpu.lib()
    n = len(c.rays)
    t, p, ins = np.full((n, 4), F(7), F), np.full((n, 4), 7, np.uint32), np.full((n, 4), 7, np.uint32)
    bary = np.full((n, 4, 2), F(7), F)
    cnt = np.full(n, 7, np.uint32)
    junk = np.zeros(max(n, 16) * 3, F)

    def args(tl_):
        a = gpu.TlasMultiHitArgs() if tl_ else gpu.BvhMultiHitArgs()
        a.m.base.rays, a.m.base.num_rays, a.m.base.tmin, a.m.base.tmax = c.rays.ctypes.data, n, 0.001, 10000.0
        a.m.base.t, a.m.base.prim, a.m.count, a.m.max_hits, a.bary = t.ctypes.data, p.ctypes.data, cnt.ctypes.data, 4, bary.ctypes.data
        if tl_:
            a.instance = ins.ctypes.data
        return a

    for tl_, h, fns in ((False, bvhs("cube")[0].h, (L.vx_bvh_trace_multi, L.vx_bvh_trace_multi_device)),
                        (True, tlas().h, (L.vx_tlas_trace_multi, L.vx_tlas_trace_multi_device))):
        cursor = ("after_t", "after_prim") + (("after_instance",) if tl_ else ())
        for fn in fns:
            assert fn(None, C.byref(args(tl_))) == INVALID_ARG
            assert fn(h, None) == INVALID_ARG
            for k in (0, 33, 0xFFFFFFFF):
                a = args(tl_)
                a.m.max_hits = k
                assert fn(h, C.byref(a)) == INVALID_ARG, k
            for given in [s for i in range(1, len(cursor)) for s in itertools.combinations(cursor, i)]:   # an incomplete cursor
                a = args(tl_)
                for f in given:
                    setattr(a if f == "after_instance" else a.m, f, junk.ctypes.data)
                assert fn(h, C.byref(a)) == INVALID_ARG, given
            for field in ("normal", "shadowed", "hits", "num_hits"):
                a = args(tl_)
                setattr(a.m.base, field, junk.ctypes.data)
                assert fn(h, C.byref(a)) == INVALID_ARG, field
            a = args(tl_)
            a.m.base.any_hit = 1
            assert fn(h, C.byref(a)) == INVALID_ARG
            a = args(tl_)
            a.m.base.rays = None     # rays announced, but neither a buffer nor a camera
            assert fn(h, C.byref(a)) == INVALID_ARG
    assert (t == F(7)).all() and (p == 7).all() and (ins == 7).all() and (bary == F(7)).all() and (cnt == 7).all()


def test_default_paths_queue_no_mesh_multihit_kernel(gpu):
    v, t = vx_scenes.blob()
    mesh = gpu.Mesh.from_arrays(v, t)
    gpu.profile_enable(True)
    gpu.profile_reset()
    g = gpu.Grid.voxelize(mesh, F(2.0 / 64))
    d = g.describe()
    rays = vx_scenes.random_rays(1000, d["bbox_min"], d["bbox_max"], seed=1)
    g.trace(rays)
    b = mesh.bvh()
    b.trace(rays)
    tl = gpu.Tlas([b], gpu.instances([np.eye(3, 4).reshape(12)]))
    tl.trace(rays)
    names = list(gpu.profile_read())
    assert "k_walk" in names and "k_bvh_trace" in names and "k_tlas_trace" in names and not any("multihit" in n for n in names), names
    gpu.profile_reset()
    b.trace_multi(rays, max_hits=8)
    b.trace_multi(rays, max_hits=32)
    tl.trace_multi(rays, max_hits=4)
    prof = gpu.profile_read()   # (kernel names come without their template arguments)
    gpu.profile_enable(False)
    assert prof["k_bvh_multihit"][1] == 2 and prof["k_tlas_multihit"][1] == 1 and "k_bvh_trace" not in prof and "k_tlas_trace" not in prof, prof


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------
def run(cmd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = PKG + ":" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)


def test_cli_mesh_xray(gpu, tmp_path):
    """--mesh-xray: a 16-bit PGM of min(count, 65535) per camera ray, against Bvh.trace_multi with the camera the CLI used"""
    cv, ct = vx_scenes.cube()
    v, t = mc.layers_scene()
    v = v * F(0.5) + np.array([0.0, 1.0, -2.0], F)     # in front of the reference camera
    obj, model = tmp_path / "cube.obj", tmp_path / "layers.obj"
    vx_scenes.write_obj(str(obj), cv, ct)
    vx_scenes.write_obj(str(model), v, t)
    pgm, cam = tmp_path / "x.pgm", tmp_path / "cam.bin"
    W, H = 96, 54
    exe = os.path.join(PKG, "voxilizer")
    r = run([exe, str(obj), "0.25", "--mesh", str(model), "--mesh-xray", str(pgm), "--size", "%dx%d" % (W, H), "--camera-dump", str(cam)])
    assert r.returncode == 0 and "xray %dx%d" % (W, H) in r.stdout and "triangle crossings" in r.stdout, r.stdout
    raw = open(pgm, "rb").read()
    hdr = b"P5\n%d %d\n65535\n" % (W, H)
    assert raw.startswith(hdr) and len(raw) == len(hdr) + 2 * W * H
    img = np.frombuffer(raw[len(hdr):], ">u2").reshape(H, W)
    cm = np.fromfile(cam, F)
    b = gpu.Mesh.from_arrays(v, t).bvh()
    cnt = b.trace_multi(camera=(cm[:16], cm[16:], W, H), max_hits=1, want=("count",))["count"].reshape(H, W)
    assert np.array_equal(img, np.minimum(cnt, 65535))
    assert cnt.max() >= 4 and (cnt == 0).any()
    # every earlier command line behaves as before: --mesh alone still needs --render, --mesh-xray needs --mesh
    r = run([exe, str(obj), "0.25", "--mesh", str(model)])
    assert r.returncode == 2 and "--mesh needs --render" in r.stdout
    r = run([exe, str(obj), "0.25", "--mesh-xray", str(pgm)])
    assert r.returncode == 2 and "--mesh-xray" in r.stdout
