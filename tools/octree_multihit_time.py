#!/usr/bin/env python3
"""Device timings of the multi-hit query on the octree (vx_octree_trace_multi_device), one JSON line.  Scenes: the atrium (BASELINE
configs[2]) at 512^3 with the 1M random rays bench.py draws, and the two-cluster scene of tests/test_gpu_octree_trace.py (more than 2^37
cells: no dense grid exists) with 1M rays aimed at the clusters.  Per scene, each the median over --reps calls (after warm-up) of device
events recorded around the call on the octree's stream:
  multi_k1, multi_k8                the lists without `count` (the ray may stop early)
  multi_k8_count, multi_k32_count   with `count` (the ray visits every node its interval enters)
  octree_ms                         vx_octree_trace_ex_device with t only: k_octree_trace, on the same rays
  grid_multi_k8_ms, grid_multi_k8_count_ms   k_multihit on the Bool grid of the same scene, where one exists; same_count: its counts are the octree's
  mean_count, max_count             voxels per ray
   usage: octree_multihit_time.py [--reps 10] [--max-items 16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402
from multihit_time import median_ms  # noqa: E402
from octree_trace_time import aimed_rays, two_cluster_mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-items", type=int, default=16)
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("octree_multihit_time.py needs a HIP device")
    res = {"reps": a.reps, "max_items": a.max_items}
    n = 1_000_000
    for scene in ("atrium262k@512^3", "two_clusters_6008^3"):
        if scene.startswith("atrium"):
            v, t = vx_scenes.scene("atrium262k")
            vs = np.float32(32.0 / 512)
            rays = vx_scenes.random_rays(n, v.min(0), v.max(0), seed=2)
        else:
            v, t = two_cluster_mesh()
            vs = np.float32(1.0)
            rays = aimed_rays(n, v)
        mesh = voxhip.Mesh.from_arrays(v, t)
        tree = voxhip.Octree(mesh, vs, max_items=a.max_items)
        grid = voxhip.Grid.voxelize(mesh, vs) if scene.startswith("atrium") else None
        d_r = torch.from_numpy(rays).cuda()
        d_t = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        d_p = torch.empty((n, 32), dtype=torch.int32, device="cuda")
        d_c = torch.empty(n, dtype=torch.int32, device="cuda")

        def multi(h, k, count):
            return lambda: h.trace_multi_device(d_r.data_ptr(), n, k, d_t.data_ptr(), d_p.data_ptr(), d_c.data_ptr() if count else None)

        w = {"items": tree.num_items, "nodes": tree.num_nodes,
             "multi_k1_ms": median_ms(multi(tree, 1, False), a.reps), "multi_k8_ms": median_ms(multi(tree, 8, False), a.reps),
             "multi_k8_count_ms": median_ms(multi(tree, 8, True), a.reps), "multi_k32_count_ms": median_ms(multi(tree, 32, True), a.reps)}
        cnt = d_c.cpu().numpy().view(np.uint32).copy()
        w["mean_count"], w["max_count"] = round(float(cnt.mean()), 3), int(cnt.max())
        w["octree_ms"] = median_ms(lambda: tree.trace_device(d_r.data_ptr(), n, t_ptr=d_t.data_ptr()), a.reps)
        if grid is not None:
            w["grid_multi_k8_ms"] = median_ms(multi(grid, 8, False), a.reps)
            w["grid_multi_k8_count_ms"] = median_ms(multi(grid, 8, True), a.reps)
            w["same_count"] = bool(np.array_equal(d_c.cpu().numpy().view(np.uint32), cnt))
        res[scene] = w
        del d_r, d_t, d_p, d_c, tree, grid
    print(json.dumps(res))


if __name__ == "__main__":
    main()
