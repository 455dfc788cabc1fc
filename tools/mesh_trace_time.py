#!/usr/bin/env python3
"""Triangle BVH timings, one JSON line: the BVH build (vx_bvh_build_into, host wall after warm-up, median of --reps) on the atrium
(BASELINE configs[2], 261k triangles) and on the configs[4] soup (10M triangles); k_bvh_trace (vx_profile_* events) at 1M and 8M random
rays (drawn as bench.py draws them) and for the interior 1280x720 camera of vx_scenes.INTERIOR_CAMERAS[0]; k_walk on the Bool grid of the
atrium at 512^3 on the same rays, for context.
   usage: mesh_trace_time.py [--reps 10] [--max-leaf 0] [--no-soup]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402
from octree_trace_time import kernel_ms  # noqa: E402


def build_ms(b, mesh, reps):
    b.build_into(mesh)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.build_into(mesh)                      # returns after the build's last kernel (it reads the node count back)
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-leaf", type=int, default=0)
    ap.add_argument("--no-soup", action="store_true")
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("mesh_trace_time.py needs a HIP device")
    out = {"scene": "atrium262k", "max_leaf": a.max_leaf}
    v, t = vx_scenes.scene("atrium262k")
    mesh = voxhip.Mesh.from_arrays(v, t)
    b = mesh.bvh(a.max_leaf)
    out["triangles"] = b.num_triangles
    out["nodes"] = b.num_nodes
    out["height"] = b.height
    out["ill_conditioned"] = b.num_ill_conditioned
    out["build_ms_atrium"] = round(build_ms(b, mesh, a.reps), 3)
    g = voxhip.Grid.voxelize(mesh, np.float32(32.0 / 512))
    d = g.describe()
    for n in (1_000_000, 8_000_000):
        rays = vx_scenes.random_rays(n, d["bbox_min"], d["bbox_max"], seed=2)
        dr = torch.from_numpy(rays).cuda()
        dt = torch.empty(n, dtype=torch.float32, device="cuda")
        dp = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = kernel_ms("k_bvh_trace", lambda: b.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr()), a.reps)
        hits = int((dt > 0).sum().item())
        wms = kernel_ms("k_walk", lambda: g.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr()), a.reps)
        k = "%dM" % (n // 1_000_000)
        out["bvh_trace_ms_" + k] = round(ms, 4)
        out["bvh_grays_" + k] = round(n / ms / 1e6, 3)
        out["bvh_hit_rate_" + k] = round(hits / n, 4)
        out["walk_ms_" + k] = round(wms, 4)
        del dr, dt, dp
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0])
    W, H = 1280, 720
    dt = torch.empty(W * H, dtype=torch.float32, device="cuda")
    dp = torch.empty(W * H, dtype=torch.int32, device="cuda")
    ms = kernel_ms("k_bvh_trace", lambda: b.trace_device(None, 0, dt.data_ptr(), dp.data_ptr(), camera=(vi, pi, W, H)), a.reps)
    out["bvh_trace_ms_camera"] = round(ms, 4)
    out["bvh_grays_camera"] = round(W * H / ms / 1e6, 3)
    out["bvh_hit_rate_camera"] = round(float((dt > 0).float().mean().item()), 4)
    if not a.no_soup:
        v, t = vx_scenes.soup(10_000_000, 4, edge=1.5 / 2048)     # BASELINE configs[4]
        sm = voxhip.Mesh.from_arrays(v, t)
        del v, t
        sb = sm.bvh(a.max_leaf)
        out["build_ms_soup10M"] = round(build_ms(sb, sm, max(3, a.reps // 3)), 3)
        out["nodes_soup10M"] = sb.num_nodes
        out["height_soup10M"] = sb.height
        out["ill_conditioned_soup10M"] = sb.num_ill_conditioned
    print(json.dumps(out))


if __name__ == "__main__":
    main()
