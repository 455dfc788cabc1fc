#!/usr/bin/env python3
"""Device timings of the multi-hit query (vx_trace_multi_device), one JSON line.  Scene: the atrium (BASELINE configs[2]) voxelized at 512^3
as a Bool grid.  Workloads: the 1M random rays bench.py draws, and the interior camera vx_scenes.INTERIOR_CAMERAS[0] at 1280x720.  Per
workload, each the median over --reps calls (after warm-up) of device events recorded around the call on the grid's stream:
  multi_k1, multi_k8          the lists without `count` (the ray may stop early)
  multi_k8_count, multi_k32_count   with `count` (the ray walks its whole interval)
  walk_ms                     vx_trace_device with t only: k_walk alone, on the same rays
  octree_ms                   vx_octree_trace_ex_device with t only: k_octree_trace, on the same rays
  mean_count, max_count       hits per ray
   usage: multihit_time.py [--reps 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402

VS = 32.0 / 512


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(float(np.median([a.elapsed_time(b) for a, b in ev])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("multihit_time.py needs a HIP device")
    v, t = vx_scenes.scene("atrium262k")
    mesh = voxhip.Mesh.from_arrays(v, t)
    grid = voxhip.Grid.voxelize(mesh, np.float32(VS))
    tree = voxhip.Octree(mesh, np.float32(VS))
    rays = torch.from_numpy(vx_scenes.random_rays(1_000_000, v.min(0), v.max(0), seed=2)).cuda()
    W, H = 1280, 720
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=W / H)
    res = {"scene": "atrium262k@512^3", "reps": a.reps}
    for name, n, src in (("random_1m", rays.shape[0], dict(rays_ptr=rays.data_ptr(), nrays=rays.shape[0])),
                         ("interior0_1280x720", W * H, dict(rays_ptr=None, nrays=0, camera=(vi, pi, W, H)))):
        d_t = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        d_p = torch.empty((n, 32), dtype=torch.int32, device="cuda")
        d_c = torch.empty(n, dtype=torch.int32, device="cuda")

        def multi(k, count):
            return lambda: grid.trace_multi_device(max_hits=k, t_ptr=d_t.data_ptr(), prim_ptr=d_p.data_ptr(), count_ptr=d_c.data_ptr() if count else None, **src)

        w = {"multi_k1_ms": median_ms(multi(1, False), a.reps), "multi_k8_ms": median_ms(multi(8, False), a.reps),
             "multi_k8_count_ms": median_ms(multi(8, True), a.reps), "multi_k32_count_ms": median_ms(multi(32, True), a.reps)}
        cnt = d_c.cpu().numpy().view(np.uint32)
        w["mean_count"], w["max_count"] = round(float(cnt.mean()), 3), int(cnt.max())
        if "camera" in src:
            w["walk_ms"] = median_ms(lambda: grid.trace_primary_device(vi, pi, W, H, d_t.data_ptr()), a.reps)
            w["octree_ms"] = median_ms(lambda: tree.trace_device(None, 0, t_ptr=d_t.data_ptr(), camera=(vi, pi, W, H)), a.reps)
        else:
            w["walk_ms"] = median_ms(lambda: grid.trace_device(rays.data_ptr(), n, d_t.data_ptr()), a.reps)
            w["octree_ms"] = median_ms(lambda: tree.trace_device(rays.data_ptr(), n, t_ptr=d_t.data_ptr()), a.reps)
        res[name] = w
        del d_t, d_p, d_c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
