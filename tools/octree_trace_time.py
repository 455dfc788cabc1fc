#!/usr/bin/env python3
"""Ray rate on the octree: k_octree_trace (vx_octree_trace_ex_device) next to k_walk on the Bool grid of the same scene, one JSON line.
   Scene: BASELINE configs[2], atrium262k at exactly 512^3 (voxel size 32/512, as bench.py builds it); random rays as bench.py draws them.
   Times are vx_profile_* events of the named kernel after warm-up; the octree build time is host wall around vx_octree_build.
   --sparse: the two-cluster scene of tests/test_gpu_octree_trace.py (> 2^37 cells: no dense grid exists), 1M rays aimed at the
   clusters, octree only.
   usage: octree_trace_time.py [--sparse] [--reps 10] [--max-items 16]"""
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


def kernel_ms(name, run, reps):
    """mean ms per launch of kernel `name` over `reps` calls of run(), after two warm-up calls"""
    run(); run()
    torch.cuda.synchronize()
    voxhip.profile_select(name)
    voxhip.profile_reset()
    voxhip.profile_enable(True)
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    voxhip.profile_enable(False)
    voxhip.profile_select(None)
    ms, n = voxhip.profile_read().get(name, (0.0, 0))
    if not n:
        raise RuntimeError("no %s launch was timed" % name)
    return ms / n


def octree_run(o, dr, n, dt, dp):
    return lambda: o.trace_device(dr.data_ptr(), n, dt.data_ptr(), dp.data_ptr())


def two_cluster_mesh(span=6000.0):
    va, ta = vx_scenes.rotated_cube(half=5.0, offset=(8.0, 8.0, 8.0))
    vb, tb = vx_scenes.rotated_cube(half=5.0, angles=(0.11, 0.83, 0.47), offset=(span, span, span))
    return np.concatenate([va, vb]).astype(np.float32), np.concatenate([ta, tb + len(va)]).astype(np.int32)


def aimed_rays(n, v, seed=4):
    """the two-cluster scene's rays: from anywhere in the box, half at each cluster (random rays there almost never hit anything)"""
    rng = np.random.default_rng(seed)
    src = v.min(0) + rng.uniform(0, 1, (n, 3)) * (v.max(0) - v.min(0))
    tgt = np.where(rng.random((n, 1)) < 0.5, np.array([8.0, 8.0, 8.0]), np.array([6000.0, 6000.0, 6000.0])) + rng.uniform(-6, 6, (n, 3))
    d = tgt - src
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([src, d], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-items", type=int, default=16)
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("octree_trace_time.py needs a HIP device")
    if a.sparse:
        v, t = two_cluster_mesh()
        vs = np.float32(1.0)
        sizes = [1_000_000]
        scene = "two_clusters_6008^3"
    else:
        v, t = vx_scenes.scene("atrium262k")
        vs = np.float32(32.0 / 512)
        sizes = [1_000_000, 8_000_000]
        scene = "atrium262k_512^3"
    mesh = voxhip.Mesh.from_arrays(v, t)
    voxhip.Octree(mesh, vs, max_items=a.max_items).free()  # warm-up: code objects, pool
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = voxhip.Octree(mesh, vs, max_items=a.max_items)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    out = {"scene": scene, "max_items": a.max_items, "octree_build_ms": round(build_ms, 3), "items": o.num_items, "nodes": o.num_nodes}
    g = None if a.sparse else voxhip.Grid.voxelize(mesh, vs)
    for n in sizes:
        rays = aimed_rays(n, v) if a.sparse else vx_scenes.random_rays(n, v.min(0), v.max(0), seed=2)
        dr = torch.from_numpy(rays).cuda()
        dt = torch.empty(n, dtype=torch.float32, device="cuda")
        dp = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = kernel_ms("k_octree_trace", octree_run(o, dr, n, dt, dp), a.reps)
        tag = "%dM" % (n // 1_000_000)
        out["k_octree_trace_us_" + tag] = round(ms * 1e3, 2)
        out["octree_grays_s_" + tag] = round(n / (ms * 1e-3) / 1e9, 4)
        out["octree_hits_" + tag] = int((dt > 0).sum().item())
        if g is not None:
            gt = torch.empty(n, dtype=torch.float32, device="cuda")
            wms = kernel_ms("k_walk", lambda: g.trace_device(dr.data_ptr(), n, gt.data_ptr()), a.reps)
            out["k_walk_us_" + tag] = round(wms * 1e3, 2)
            out["walk_grays_s_" + tag] = round(n / (wms * 1e-3) / 1e9, 4)
            out["same_t_" + tag] = bool(torch.equal(dt.view(torch.int32), gt.view(torch.int32)))
        del dr, dt, dp
    print(json.dumps(out))


if __name__ == "__main__":
    main()
