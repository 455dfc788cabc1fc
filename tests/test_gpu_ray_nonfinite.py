"""GPU tests of the non-finite ray rule (include/voxhip.h, "Non-finite rays"): a ray with NaN or +-Inf in any component
is a miss on every ray query -- grid (k_walk in its LDS / global-mip, donating / non-donating and WIDE variants, the rank epilogue, k_rank,
k_multihit), octree, triangle BVH, TLAS, their multi-hit kernels, camera rays and frames -- and changes nothing for the finite rays beside
it.  Batches of tests/ray_nonfinite.py: poisoned copies of hitting rays mixed with finite rays; expected values are the rule on the
poisoned rays and the unchanged brute force of tests/ray_extremes.py on the finite ones, bit for bit.  tests/test_ray_nonfinite_cpu.py
checks the rays, the batches and the references themselves."""
import numpy as np
import pytest

import ray_extremes as rx
import ray_nonfinite as nf
from test_gpu_configs import env
from test_gpu_ray_extremes import LEAVES, WANT, WANT_MULTI, Ref, handle, same

pytestmark = pytest.mark.gpu

F = np.float32
NAN = np.nan
# (structure, scene, argument): the smallest scenes that reach every kernel variant (the wide grid is the only one that selects k_walk's WIDE ones)
TRACERS = [("grid", "rotcube", None), ("grid", "wide", None), ("octree", "rotcube", None)] + \
          [("bvh", n, l) for n in rx.BVH_SCENES for l in LEAVES] + [("tlas", "tlas", l) for l in LEAVES]
IDS = ["%s-%s%s" % (k, n, "" if a is None else "-leaf%d" % a) for k, n, a in TRACERS]
_refs = {}


class Case:
    """a tracer, and its references on the pool (the finite rays of tests/ray_nonfinite.py) over [0, +inf], computed once per module"""

    def __init__(self, vx, kind, name, arg):
        h = handle(vx, kind, name, arg)
        self.tracer = h[0] if kind == "tlas" else h
        self.kind = "grid" if kind == "octree" else kind            # the reference's kind
        self.name, self.what = name, "%s %s %s" % (kind, name, arg)
        self.device = kind
        key = (kind, name)
        if key not in _refs:
            ref = Ref(self.kind, name, boxes=self.tracer.aabbs() if kind == "octree" else None)
            closest = ref.closest(nf.POOL, *nf.OPEN)
            r = {"closest": closest, "any": {"shadowed": ref.any(nf.POOL, *nf.OPEN, closest_t=closest["t"])}}
            if ref.has_multi:
                r["multi"] = ref.multi(nf.POOL, *nf.OPEN)
            _refs[key] = r
        self.ref = _refs[key]
        self.want = WANT[self.kind]
        self.has_multi = "multi" in self.ref

    def batch(self, which, multi=False):
        return nf.batch(self.kind, self.name, which, multi)

    def closest(self, rays, want=None, **kw):
        kw = dict(dict(tmin=nf.OPEN[0], tmax=nf.OPEN[1]), **kw)
        return self.tracer.trace_ex(rays, want=self.want if want is None else want, **kw)

    def multi(self, rays, **kw):
        kw = dict(dict(tmin=nf.OPEN[0], tmax=nf.OPEN[1]), **kw)
        return self.tracer.trace_multi(rays, max_hits=nf.K, want=WANT_MULTI[self.kind], **kw)

    def expected(self, src, what="closest"):
        ref = self.ref[what]
        if what == "closest" and self.kind != "grid":     # (mesh normals are compared with the tracer's own on the finite rays alone)
            ref = {k: v for k, v in ref.items() if k != "normal"}
        return nf.masked(src, ref)


@pytest.fixture(params=TRACERS, ids=IDS)
def case(request, gpu):
    return Case(gpu, *request.param)


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def device_outputs(case, rays):
    """the device entry point with the compacted hit list -> (dict of per-ray outputs, hit records sorted by ray, num_hits)"""
    import torch
    n = len(rays)
    dr = torch.from_numpy(np.array(rays, np.float32)).cuda()
    dt = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    dp = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dh = torch.zeros(n * 3, dtype=torch.int32, device="cuda")
    dn = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    extra = {}
    torch.cuda.synchronize()
    args = (dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr())
    kw = dict(hits_ptr=dh.data_ptr(), nhits_ptr=dn.data_ptr(), tmin=nf.OPEN[0], tmax=nf.OPEN[1])
    if case.device == "tlas":
        extra = {"instance": torch.full((n,), 7, dtype=torch.int32, device="cuda"), "bary": torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")}
        case.tracer.trace_device(*args, instance_ptr=extra["instance"].data_ptr(), bary_ptr=extra["bary"].data_ptr(), **kw)
    elif case.device == "bvh":
        extra = {"bary": torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")}
        case.tracer.trace_device(*args, bary_ptr=extra["bary"].data_ptr(), **kw)
    else:
        case.tracer.trace_device(*args, **kw)
    torch.cuda.synchronize()
    out = {"t": dt.cpu().numpy(), "prim": dp.cpu().numpy().view(np.uint32)}
    for k, v in extra.items():
        out[k] = v.cpu().numpy().view(np.uint32) if k == "instance" else v.cpu().numpy()
    nh = int(dn.item())
    assert 0 <= nh <= n, nh
    hits = dh.cpu().numpy().view(np.uint32).reshape(-1, 3)[:nh]
    return out, hits[np.argsort(hits[:, 0], kind="stable")], nh


# ---- every batch on every tracer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", nf.BATCHES, ids=[str(b) for b in nf.BATCHES])
def test_batch(case, which):
    """all outputs of every query: the rule on the poisoned rays, the reference on the finite ones; num_hits and the compacted list hold
    exactly the finite hits; and the finite rays' outputs are, bit for bit, what the same tracer returns for them alone"""
    src, rays = case.batch(which)
    dead, what = src < 0, "%s batch %s" % (case.what, which)
    exp = case.expected(src)
    nhit = int((exp["t"] > 0).sum())
    # closest hit with normals (and bary)
    got = case.closest(rays)
    same(got, exp, rays, what + " closest")
    assert zero_bits(got["normal"][dead]), what + ": normal of a non-finite ray"
    assert (got["t"][dead] == -1).all() and (got["prim"][dead] == nf.MISS).all()
    # shadow query, with every output it can write
    ga = case.closest(rays, any_hit=True, want=("t", "shadowed"))
    same({"shadowed": ga["shadowed"]}, case.expected(src, "any"), rays, what + " any_hit")
    assert (ga["t"][dead] == -1).all() and np.array_equal(ga["t"] > 0, ga["shadowed"] == 1)
    # the plain entry point: num_hits
    out = case.tracer.trace(rays, *nf.OPEN)
    same({"t": out[0], "prim": out[-2]}, {"t": exp["t"], "prim": exp["prim"]}, rays, what + " trace")
    assert out[-1] == nhit, what + " num_hits"
    # the device entry point with the compacted hit list
    dev, hits, nh = device_outputs(case, rays)
    same(dev, exp, rays, what + " device")
    idx = np.flatnonzero(exp["t"] > 0)
    assert nh == nhit, what + " device num_hits"
    assert np.array_equal(hits[:, 0], idx) and np.array_equal(hits[:, 1], exp["prim"][idx]) and np.array_equal(hits[:, 2], exp["t"][idx].view(np.uint32)), \
        what + " hit list"
    # independence: a poisoned neighbour changes nothing in its wave
    alive = ~dead
    if alive.any():
        alone = case.closest(rays[alive])
        same({k: v[alive] for k, v in got.items()}, alone, rays[alive], what + " finite rays alone")
        sa = case.closest(rays[alive], any_hit=True, want=("shadowed",))["shadowed"]
        assert np.array_equal(ga["shadowed"][alive], sa), what + " finite rays alone, any_hit"
    # K = 4 multi-hit
    if case.has_multi:
        msrc, mrays = case.batch(which, multi=True)
        mdead = msrc < 0
        gm = case.multi(mrays)
        same(gm, case.expected(msrc, "multi"), mrays, what + " multi")
        assert not gm["count"][mdead].any() and (gm["t"][mdead] == -1).all() and (gm["prim"][mdead] == nf.MISS).all()
        if (~mdead).any():
            same({k: v[~mdead] for k, v in gm.items()}, case.multi(mrays[~mdead]), mrays[~mdead], what + " multi, finite rays alone")


# ---- NaN intervals ----------------------------------------------------------------------------------------------------------------------------
def test_nan_intervals(case):
    """a NaN tmin or tmax accepts nothing (a comparison with NaN fails); NaN entries of tmax_per_ray make those rays miss and leave the
    others as they were"""
    src, rays = case.batch(257)
    n, what = len(rays), case.what + " NaN interval"
    miss = nf.all_miss(n, case.want)
    for tmin, tmax in ((NAN, np.inf), (0.0, NAN), (NAN, NAN)):
        got = case.closest(rays, tmin=tmin, tmax=tmax)
        assert set(got) == set(miss)
        same(got, miss, rays, "%s [%s, %s]" % (what, tmin, tmax))
        assert not case.closest(rays, any_hit=True, want=("shadowed",), tmin=tmin, tmax=tmax)["shadowed"].any()
        assert case.tracer.trace(rays, tmin, tmax)[-1] == 0
        if case.has_multi:
            gm = case.multi(rays, tmin=tmin, tmax=tmax)
            same(gm, nf.all_miss(n, WANT_MULTI[case.kind], nf.K), rays, "%s [%s, %s] multi" % (what, tmin, tmax))
    tm = np.full(n, np.inf, F)
    tm[1:: 3] = NAN
    tm[2:: 7] = np.array([0xFFC00000], np.uint32).view(F)[0]
    src2 = np.where(np.isnan(tm), -1, src)
    assert (src2[src >= 0] < 0).any() and (src2 >= 0).any()
    got = case.closest(rays, tmin=0.0, tmax=1.0, tmax_per_ray=tm)
    same(got, case.expected(src2), rays, what + " per-ray tmax")
    sh = case.closest(rays, any_hit=True, want=("shadowed",), tmin=0.0, tmax=1.0, tmax_per_ray=tm)
    same(sh, case.expected(src2, "any"), rays, what + " per-ray tmax any_hit")
    if case.has_multi:
        msrc, mrays = case.batch(257, multi=True)
        gm = case.multi(mrays, tmin=0.0, tmax=1.0, tmax_per_ray=tm)
        same(gm, case.expected(np.where(np.isnan(tm), -1, msrc), "multi"), mrays, what + " per-ray tmax multi")


# ---- the grid's prim ranks: both routes through k_walk's rank epilogue, and none -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["rotcube", "wide"])
def test_grid_prim_ranks(gpu, name):
    """want = ("t",) alone (no rank pass), ("t", "prim") and ("prim",) alone (the waves of k_walk rank the rays of their chunks as they
    leave: lanes that retired at set-up are among them): prim is 0xFFFFFFFF for those and right for the rest"""
    case = Case(gpu, "grid", name, None)
    for which in (65, 257, "runs", "all"):
        src, rays = case.batch(which)
        exp = case.expected(src)
        for want in (("t",), ("t", "prim"), ("prim",)):
            got = case.closest(rays, want=want)
            assert set(got) == set(want)
            same(got, {k: exp[k] for k in want}, rays, "grid %s batch %s want=%s" % (name, which, want))


# ---- k_walk's other variants on the small grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds,donate", [(0, 1), (1, 0), (0, 0)])
def test_grid_forced_paths(gpu, lds, donate):
    """the mips read from global memory and / or no work donation: the same batches, t, prim and num_hits"""
    case = Case(gpu, "grid", "rotcube", None)
    with env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=donate):
        for which in nf.BATCHES:
            src, rays = case.batch(which)
            exp = case.expected(src)
            what = "grid rotcube lds=%d donate=%d batch %s" % (lds, donate, which)
            out = case.tracer.trace(rays, *nf.OPEN)
            same({"t": out[0], "prim": out[1]}, {"t": exp["t"], "prim": exp["prim"]}, rays, what)
            assert out[2] == int((exp["t"] > 0).sum()), what + " num_hits"
            same(case.closest(rays, want=("t", "prim")), {"t": exp["t"], "prim": exp["prim"]}, rays, what + " t + prim")
            sh = case.closest(rays, any_hit=True, want=("shadowed",))
            same(sh, case.expected(src, "any"), rays, what + " any_hit")


# ---- rays generated from the camera matrices ---------------------------------------------------------------------------------------------------
CAMERA_TRACERS = [("grid", "rotcube", None), ("octree", "rotcube", None), ("bvh", "floor", 0), ("tlas", "tlas", 0)]


@pytest.mark.parametrize("cam", ["nan translation", "zero projection"])
@pytest.mark.parametrize("tr", CAMERA_TRACERS, ids=[t[0] for t in CAMERA_TRACERS])
def test_camera_rays_miss(gpu, tr, cam):
    """an 8 x 8 image whose view_inverse has a NaN translation (every origin NaN), and one whose proj_inverse is all zeros (every direction
    NaN through 1 / sqrt(0)): every pixel misses, in every output"""
    h = handle(gpu, *tr)
    tracer = h[0] if tr[0] == "tlas" else h
    kind = "grid" if tr[0] == "octree" else tr[0]
    camera = nf.cameras()[cam]
    n = nf.W * nf.H
    for any_hit in (False, True):
        want = ("t", "shadowed") if any_hit else WANT[kind] + ("shadowed",)
        got = tracer.trace_ex(camera=camera, want=want, any_hit=any_hit, tmin=nf.OPEN[0], tmax=nf.OPEN[1])
        exp = nf.all_miss(n, want)
        assert set(got) == set(exp)
        for k in exp:
            assert rx.same_bits(got[k], exp[k]), "%s %s any_hit=%d: %s" % (tr[0], cam, any_hit, k)
    if hasattr(tracer, "trace_multi"):
        gm = tracer.trace_multi(camera=camera, max_hits=nf.K, tmin=nf.OPEN[0], tmax=nf.OPEN[1], want=WANT_MULTI[kind])
        exp = nf.all_miss(n, WANT_MULTI[kind], nf.K)
        for k in exp:
            assert rx.same_bits(gm[k], exp[k]), "%s %s multi: %s" % (tr[0], cam, k)


def test_camera_away_is_all_miss_and_finite(gpu):
    """the comparison camera of the frame test below: finite rays, none of which hits the grid or the mesh"""
    import oracle
    vi, pi, w, h = nf.cameras()["away"]
    assert np.isfinite(oracle.primary_rays(vi, pi, w, h)).all()
    for tr in CAMERA_TRACERS[:3]:
        t = handle(gpu, *tr).trace_ex(camera=(vi, pi, w, h), want=("t",), tmin=nf.OPEN[0], tmax=nf.OPEN[1])["t"]
        assert (t == -1).all(), tr


@pytest.mark.parametrize("cam", ["nan translation", "zero projection"])
def test_frame_of_a_nonfinite_camera(gpu, cam):
    """one 8 x 8 frame through the renderer (voxel grid + triangle BVH): the frame of a non-finite camera is the all-miss frame of a camera
    that looks away from the scene -- colours, kind bytes and shadow bytes"""
    sc = rx.mesh_scene("floor")
    mesh = gpu.Mesh.from_arrays(sc.v, sc.t)
    bvh = mesh.bvh()
    r = gpu.Renderer(handle(gpu, "grid", "rotcube"), bvh=bvh, mesh=mesh)
    cams = nf.cameras()
    want = ("rgba", "kind", "shadowed")
    away = r.render_host(cams["away"], want=want)
    assert not away["kind"].any() and not away["shadowed"].any() and (away["rgba"] == away["rgba"][0, 0]).all()
    got = r.render_host(cams[cam], want=want)
    for k in want:
        assert np.array_equal(got[k], away[k]), "%s: %s" % (cam, k)
    r.free()
