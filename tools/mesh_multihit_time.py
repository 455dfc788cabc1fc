#!/usr/bin/env python3
"""Device timings of the multi-hit query on the triangle BVH (vx_bvh_trace_multi_device), one JSON line.  Scene: the atrium (BASELINE
configs[2]) as a BVH at the default leaf size.  Workloads: the 1M random rays bench.py draws, and the interior camera
vx_scenes.INTERIOR_CAMERAS[0] at 1280x720.  Per workload, each the median over --reps calls (after warm-up) of device events recorded
around the call on the BVH's stream:
  multi_k1, multi_k8                the lists without `count` (the descent prunes against the K-th kept t)
  multi_k8_count, multi_k32_count   with `count` (the descent visits everything the ray's interval reaches)
  bvh_trace_ms                      vx_bvh_trace_ex_device with t only: k_bvh_trace, on the same rays
  mean_count, max_count             triangles per ray
   usage: mesh_multihit_time.py [--reps 10]"""
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
from multihit_time import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("mesh_multihit_time.py needs a HIP device")
    v, t = vx_scenes.scene("atrium262k")
    bvh = voxhip.Mesh.from_arrays(v, t).bvh()
    rays = torch.from_numpy(vx_scenes.random_rays(1_000_000, v.min(0), v.max(0), seed=2)).cuda()
    W, H = 1280, 720
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=W / H)
    res = {"scene": "atrium262k", "triangles": bvh.num_triangles, "height": bvh.height, "reps": a.reps}
    for name, n, src in (("random_1m", rays.shape[0], dict(rays_ptr=rays.data_ptr(), nrays=rays.shape[0])),
                         ("interior0_1280x720", W * H, dict(rays_ptr=None, nrays=0, camera=(vi, pi, W, H)))):
        d_t = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        d_p = torch.empty((n, 32), dtype=torch.int32, device="cuda")
        d_c = torch.empty(n, dtype=torch.int32, device="cuda")

        def multi(k, count):
            return lambda: bvh.trace_multi_device(max_hits=k, t_ptr=d_t.data_ptr(), prim_ptr=d_p.data_ptr(), count_ptr=d_c.data_ptr() if count else None, **src)

        w = {"multi_k1_ms": median_ms(multi(1, False), a.reps), "multi_k8_ms": median_ms(multi(8, False), a.reps),
             "multi_k8_count_ms": median_ms(multi(8, True), a.reps), "multi_k32_count_ms": median_ms(multi(32, True), a.reps)}
        cnt = d_c.cpu().numpy().view(np.uint32)
        w["mean_count"], w["max_count"] = round(float(cnt.mean()), 3), int(cnt.max())
        w["bvh_trace_ms"] = median_ms(lambda: bvh.trace_device(src["rays_ptr"], src["nrays"], t_ptr=d_t.data_ptr(), camera=src.get("camera")), a.reps)
        res[name] = w
        del d_t, d_p, d_c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
