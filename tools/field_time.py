#!/usr/bin/env python3
"""Distance-field queries (vx_field) timed on the atrium at 512^3, solid; one JSON line.  Medians of --reps calls by device events, after
warm-up, into preallocated tensors; create / update (which wait for the host) by the host's clock around the call.
  create / update   next to vx_grid_sdf_device in the same run
  sample_device     value only and value + gradient, on 1M uniformly random points of the box and on 1M coherent points (the first-hit points
                    of the 1280 x 720 interior camera rays): ns per point and the share of 8 TB/s by the algorithmic bytes (12 B in, 4 or 16 B
                    out, 32 B of corners)
  sphere_trace_device at radius 0 and 2 vs, defaults otherwise, on the interior camera rays and on 1M random rays, each beside
                    vx_trace_device on the same rays; mean and maximum steps, the STEP_LIMIT share and the step histogram (powers of two)
   usage: field_time.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402

ROOF = 8e12  # bytes/s
F = np.float32


def median_ms(f, reps):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


def median_wall_ms(f, reps):
    f()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def camera_rays(vi, pi, W, H):
    """the ray of every pixel as the ray kernels generate it"""
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    u = ((px.reshape(-1).astype(F) + F(0.5)) / F(W)).astype(F)
    v = ((py.reshape(-1).astype(F) + F(0.5)) / F(H)).astype(F)
    ndx, ndy = u * F(2) - F(1), v * F(2) - F(1)
    tg = [(pi[k] * ndx + pi[4 + k] * ndy) + F(pi[8 + k] + pi[12 + k]) for k in range(3)]
    il = F(1) / np.sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2])
    n = [t * il for t in tg]
    d = [(vi[k] * n[0] + vi[4 + k] * n[1]) + vi[8 + k] * n[2] for k in range(3)]
    o = [np.full(W * H, vi[12 + k], dtype=F) for k in range(3)]
    return np.stack(o + d, axis=1).astype(F)


def time_samples(field, label, pts, reps):
    n = len(pts)
    d_p = torch.from_numpy(pts).cuda()
    d_v = torch.empty(n, dtype=torch.float32, device="cuda")
    d_g = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    out = dict(points=label, n=n)
    for name, grad, nbytes in (("value", None, 12 + 4 + 32), ("value_gradient", d_g, 12 + 16 + 32)):
        ms = median_ms(lambda: field.sample_device(d_p.data_ptr(), n, d_v.data_ptr(), grad.data_ptr() if grad is not None else None), reps)
        out[name] = dict(ms=ms, ns_per_point=round(ms * 1e6 / n, 4), roofline_share=round(nbytes * n / (ms * 1e-3) / ROOF, 4))
    return out


def time_rays(grid, field, label, rays, vs, reps):
    n = len(rays)
    d_r = torch.from_numpy(rays).cuda()
    d_t = torch.empty(n, dtype=torch.float32, device="cuda")
    d_p = torch.empty(n, dtype=torch.int32, device="cuda")
    d_s = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = dict(rays=label, n=n)
    ms = median_ms(lambda: grid.trace_device(d_r.data_ptr(), n, d_t.data_ptr(), d_p.data_ptr()), reps)
    out["vx_trace_device"] = dict(ms=ms, mrays_per_s=round(n / (ms * 1e-3) / 1e6, 1), hit_rate=round(float((d_t > 0).float().mean().item()), 4))
    for name, radius in (("radius_0", 0.0), ("radius_2vs", float(F(2) * vs))):
        ms = median_ms(lambda: field.sphere_trace_device(d_r.data_ptr(), n, radius=radius, t_ptr=d_t.data_ptr(), steps_ptr=d_s.data_ptr(),
                                                         status_ptr=d_st.data_ptr()), reps)
        steps, status = d_s.cpu().numpy(), d_st.cpu().numpy()
        hist = np.bincount(np.ceil(np.log2(np.maximum(steps, 1))).astype(np.int64), minlength=9)
        out[name] = dict(ms=ms, mrays_per_s=round(n / (ms * 1e-3) / 1e6, 1), hit_rate=round(float((status == 1).mean()), 4),
                         step_limit_share=round(float((status == 2).mean()), 5), mean_steps=round(float(steps.mean()), 2), max_steps=int(steps.max()),
                         msteps_per_s=round(float(steps.sum()) / (ms * 1e-3) / 1e6, 1),
                         steps_histogram_le_pow2={str(1 << k): int(c) for k, c in enumerate(hist)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    v, t = vx_scenes.atrium()
    vs = F(32.0 / 512)
    g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), vs, solid=True)
    d = g.describe()
    X, Y, Z = d["dim"]
    sdf = torch.empty((Z, Y, X), dtype=torch.float32, device="cuda")
    res = dict(tool="field_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, scene="atrium solid", dim=(X, Y, Z), occupied=d["occupied"])
    res["sdf_device_ms"] = median_ms(lambda: g.sdf_device(out=sdf), a.reps)
    fields = []

    def create():
        fields.append(g.field())
        if len(fields) > 1:
            fields.pop(0).free()
    res["create_wall_ms"] = median_wall_ms(create, a.reps)
    field = fields[-1]
    res["update_wall_ms"] = median_wall_ms(lambda: field.update(g), a.reps)
    W, H = 1280, 720
    cams = [vx_scenes.camera_matrices(**c) for c in vx_scenes.INTERIOR_CAMERAS]
    cam_rays = np.concatenate([camera_rays(np.asarray(vi, F).reshape(-1), np.asarray(pi, F).reshape(-1), W, H) for vi, pi in cams])
    tt = g.trace(cam_rays, want_prim=False)[0]
    hit = tt > 0
    coherent = (cam_rays[hit, :3] + tt[hit, None] * cam_rays[hit, 3:]).astype(F)[:1_000_000]
    lo, hi = d["origin"], d["origin"] + np.array([X, Y, Z], F) * vs
    uniform = (np.random.default_rng(1).random((1_000_000, 3)) * (hi - lo) + lo).astype(F)
    res["sample_device"] = [time_samples(field, "uniform in the box", uniform, a.reps), time_samples(field, "first-hit points of the interior camera rays", coherent, a.reps)]
    res["sphere_trace_device"] = [time_rays(g, field, "interior camera, %dx%d" % (W, H), cam_rays[:W * H], vs, a.reps),
                                  time_rays(g, field, "random_1m", vx_scenes.random_rays(1_000_000, v.min(0), v.max(0), seed=2), vs, a.reps)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
