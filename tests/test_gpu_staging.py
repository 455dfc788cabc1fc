"""GPU tests of the host variants' staging through blocks a handle keeps (vx_field's st_* blocks, the grid's near_val / dist_out / morph_out):
queries of growing and shrinking sizes share the blocks, every host output equals the _device variant's bit for bit, a repeated round asks
the pool for nothing, and a refused or empty call asks it for nothing at all."""
import ctypes as C
import gc

import numpy as np
import pytest

import distance_ref as dr
import field_cases as fc
import poses_cases as pc
from test_gpu_solid import write_mask

pytestmark = pytest.mark.gpu

F = np.float32
INVALID_ARG = 1
DIMS = (33, 9, 7)
SAMPLE = dict(value=(F, 1), gradient=(F, 3), occupied=(np.uint8, 1))
TRACE = dict(t=(F, 1), clearance=(F, 1), steps=(np.uint32, 1), status=(np.uint8, 1))
POSES = dict(clearance=(F, 1), point=(np.uint32, 1), count=(np.uint32, 1), position=(F, 3), gradient=(F, 3))


def masked_grid(gpu):
    """33 x 9 x 7 at vs 0.37 with about 10 % of the cells occupied"""
    X, Y, Z = DIMS
    cells = np.random.default_rng(11).random((Z, Y, X)) < 0.1
    g = gpu.Grid.create(gpu.GRID_BOOL, X, Y, Z, fc.VS_ODD, fc.ORG)
    write_mask(g, dr.pack(cells))
    g.refresh()
    return g


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d bytes differ" % (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()))


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_outputs(n, spec, want):
    """name -> an uninitialised device tensor per wanted output (uint32 as int32: the same bits)"""
    import torch
    kinds = {F: torch.float32, np.uint32: torch.int32, np.uint8: torch.uint8}
    return {k: torch.empty((n, spec[k][1]) if spec[k][1] > 1 else n, dtype=kinds[spec[k][0]], device="cuda") for k in want}


def down(outs, spec):
    import torch
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(spec[k][0]) for k, t in outs.items()}


def field_round(org, vs):
    """the six queries of one round: (what, host call, _device call), each call f -> dict of numpy outputs"""
    pts257, pts64 = fc.random_points(DIMS, org, vs, 257, 1), fc.random_points(DIMS, org, vs, 64, 3)
    rays1024, rays100 = fc.random_rays(DIMS, org, vs, 1024, 2), fc.random_rays(DIMS, org, vs, 100, 4)
    rng = np.random.default_rng(5)
    tpr, rpr = (rng.random(1024) * 30).astype(F), (rng.random(1024) * 2 * vs).astype(F)
    body32, radii32 = pc.body(32, vs, 6)
    body70, _ = pc.body(70, vs, 7)
    xf300, xf5 = pc.transforms(DIMS, org, vs, 300, 8), pc.transforms(DIMS, org, vs, 5, 9)

    def sample(pts, want):
        def dev(f):
            o, dp = device_outputs(len(pts), SAMPLE, want), up(pts)
            f.sample_device(dp.data_ptr(), len(pts), **{k + "_ptr": t.data_ptr() for k, t in o.items()})
            return down(o, SAMPLE)
        return lambda f: f.sample(pts, want=want), dev

    def trace(rays, want, tmax_per_ray=None, radius_per_ray=None):
        def dev(f):
            o, dr_ = device_outputs(len(rays), TRACE, want), up(rays)
            keep = [up(x) if x is not None else None for x in (tmax_per_ray, radius_per_ray)]
            f.sphere_trace_device(dr_.data_ptr(), len(rays), tmax_per_ray_ptr=keep[0].data_ptr() if keep[0] is not None else None,
                                  radius_per_ray_ptr=keep[1].data_ptr() if keep[1] is not None else None,
                                  **{k + "_ptr": t.data_ptr() for k, t in o.items()})
            return down(o, TRACE)
        return lambda f: f.sphere_trace(rays, tmax_per_ray=tmax_per_ray, radius_per_ray=radius_per_ray, want=want), dev

    def poses(body, xf, radii, want):
        def dev(f):
            o, db, dx = device_outputs(len(xf), POSES, want), up(body), up(xf)
            dr_ = up(radii) if radii is not None else None
            f.poses_device(db.data_ptr(), len(body), dx.data_ptr(), len(xf), radii_ptr=dr_.data_ptr() if dr_ is not None else None, margin=0.1,
                           **{k: t.data_ptr() for k, t in o.items()})
            return down(o, POSES)
        return lambda f: f.poses(body, xf, radii=radii, margin=0.1, want=want), dev

    return [("sample, 257 points", *sample(pts257, tuple(SAMPLE))),
            ("sphere_trace, 1024 rays", *trace(rays1024, tuple(TRACE), tpr, rpr)),
            ("poses, 32 spheres x 300", *poses(body32, xf300, radii32, tuple(POSES))),
            ("sample, 64 points", *sample(pts64, ("gradient",))),
            ("sphere_trace, 100 rays", *trace(rays100, ("status",))),
            ("poses, 70 points x 5", *poses(body70, xf5, None, ("count",)))]


def test_field_queries_share_kept_blocks_across_sizes(gpu):
    g = masked_grid(gpu)
    g.sdf()
    gc.collect()  # (the handles that other tests dropped without free() go now, not halfway through the count)
    live0 = gpu.device_live_blocks()
    f = g.field()
    calls = field_round(fc.ORG, fc.VS_ODD)
    want = [dev(f) for _, _, dev in calls]  # the _device variants' outputs, computed once
    assert (want[1]["status"] == gpu.FIELD_HIT).any() and (want[1]["status"] == gpu.FIELD_MISS).any() and want[2]["count"].any()
    for rnd in range(2):
        n0 = gpu.device_allocations()
        for (what, host, _), ref in zip(calls, want):
            got = host(f)
            assert list(got) == list(ref), what
            for k in ref:
                same_bits(got[k].reshape(ref[k].shape), ref[k], "%s, %s, round %d" % (what, k, rnd))
        if rnd:
            assert gpu.device_allocations() == n0, "the second round asked the pool for %d blocks" % (gpu.device_allocations() - n0)
    f.free()
    assert gpu.device_live_blocks() == live0
    g.free()


def test_grid_analysis_entries_share_kept_blocks(gpu):
    import torch
    g = masked_grid(gpu)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    values, fill = np.arange(n, dtype=np.uint32) ^ np.uint32(0x5A5A1234), 0xABCD0123

    def bits(t):
        torch.cuda.synchronize()
        return t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.uint32 else t.cpu().numpy()

    want = [("sdf", bits(g.sdf_device())),
            ("nearest_gather", bits(g.nearest_gather_device(up(values.view(np.int32)), fill=fill))),
            ("distance_sq inside", bits(g.distance_sq_device(inside=True))),
            ("morph_mask dilate 2", bits(g.morph_mask_device(gpu.MORPH_DILATE, 2)))]
    host = [g.sdf, lambda: g.nearest_gather(values, fill=fill), lambda: g.distance_sq(inside=True), lambda: g.morph_mask(gpu.MORPH_DILATE, 2)]
    assert (want[1][1] != fill).any() and want[2][1].any() and want[3][1].any()
    for rnd in range(2):
        n0 = gpu.device_allocations()
        for call, (what, ref) in zip(host, want):
            same_bits(call().reshape(ref.shape), ref, "%s, round %d" % (what, rnd))
        if rnd:
            assert gpu.device_allocations() == n0, "the second round asked the pool for %d blocks" % (gpu.device_allocations() - n0)
    g.free()


def test_refused_and_empty_field_calls_touch_nothing(gpu):
    L = gpu.lib()
    g = masked_grid(gpu)
    f = g.field()  # (no query yet: none of its staging blocks exists)
    n = 16
    pts, rays = fc.random_points(DIMS, fc.ORG, fc.VS_ODD, n, 1), fc.random_rays(DIMS, fc.ORG, fc.VS_ODD, n, 2)
    xf = pc.transforms(DIMS, fc.ORG, fc.VS_ODD, n, 3)
    out = np.zeros(3 * n, dtype=F)

    def sample_args(num=n, outputs=True):
        a = gpu.FieldSampleArgs()
        a.points, a.num_points = pts.ctypes.data, num
        if outputs:
            a.value = out.ctypes.data
        return a

    def trace_args(num=n, **kw):
        a = gpu.FieldTraceArgs()
        a.rays, a.num_rays, a.tmin, a.tmax, a.t = rays.ctypes.data, num, 0.001, 10000.0, out.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def pose_args(num=n, margin=0.0, outputs=True):
        a = gpu.FieldPoseArgs()
        a.points, a.num_points, a.transforms, a.num_poses, a.margin = pts.ctypes.data, n, xf.ctypes.data, num, margin
        if outputs:
            a.clearance = out.ctypes.data
        return a

    gc.collect()  # (as above)
    n0, live0 = gpu.device_allocations(), gpu.device_live_blocks()
    for sample, trace, poses in ((L.vx_field_sample, L.vx_field_sphere_trace, L.vx_field_poses),
                                 (L.vx_field_sample_device, L.vx_field_sphere_trace_device, L.vx_field_poses_device)):
        assert sample(f.h, C.byref(sample_args(outputs=False))) == INVALID_ARG
        assert trace(f.h, C.byref(trace_args(step_scale=2.0))) == INVALID_ARG
        assert trace(f.h, C.byref(trace_args(max_steps=65536))) == INVALID_ARG
        assert poses(f.h, C.byref(pose_args(margin=float("nan")))) == INVALID_ARG
        assert poses(f.h, C.byref(pose_args(outputs=False))) == INVALID_ARG
        assert sample(f.h, C.byref(sample_args(num=0))) == 0
        assert trace(f.h, C.byref(trace_args(num=0))) == 0
        assert poses(f.h, C.byref(pose_args(num=0))) == 0
    assert gpu.device_allocations() == n0 and gpu.device_live_blocks() == live0
    assert not out.any()
    f.free()
    g.free()
