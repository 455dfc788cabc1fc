#!/usr/bin/env python3
"""The feature transform (vx_grid_nearest_device) timed by device events beside its yardstick, vx_grid_distance_sq_device, in the same
run; one JSON line.  Per case: the median of --reps calls of each, their ratio, the algorithmic bytes both move (x pass: the mask in, N x 4 B
out; y and z passes: N x 4 B in and out, in place: N/8 + 4N + 2 x 8N) and their share of an 8 TB/s roofline, the fused gather
(vx_grid_nearest_gather_device, N x 4 B of values read at random on top), and the per-kernel times of one call of each (vx_profile_*).  The
envelopes' stacks (8 B per entry pushed and read back) are not in the algorithmic bytes: they depend on the data.
Cases, as tools/distance_time.py: the blob at 256^3 and 512^3, surface and solid; the atrium at 512^3; a 4 x 4 x 65536 mask with one cell
in 5000 occupied.
   usage: nearest_time.py [--reps 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import solid_ref  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402

ROOF = 8e12  # bytes/s


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


def kernels(f):
    voxhip.profile_reset()
    voxhip.profile_enable(True)
    f()
    torch.cuda.synchronize()
    voxhip.profile_enable(False)
    return {name: [round(ms, 4), n] for name, (ms, n) in voxhip.profile_read().items() if "dist" in name or "near" in name}


def time_grid(label, g, reps):
    X, Y, Z = g.describe()["dim"]
    n = X * Y * Z
    dsq = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    near = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    t_sq = median_ms(lambda: g.distance_sq_device(out=dsq), reps)
    t_near = median_ms(lambda: g.nearest_device(out=near), reps)
    t_in = median_ms(lambda: g.nearest_device(out=near, inside=True), reps)
    t_sq_in = median_ms(lambda: g.distance_sq_device(out=dsq, inside=True), reps)
    t_gather = median_ms(lambda: g.nearest_gather_device(vals, out=near), reps)
    b = n / 8 + 4 * n + 2 * 8 * n
    return dict(case=label, dim=(X, Y, Z), occupied=g.describe()["occupied"], distance_sq_ms=t_sq, nearest_ms=t_near,
                ratio=round(t_near / t_sq, 3), distance_sq_inside_ms=t_sq_in, nearest_inside_ms=t_in, ratio_inside=round(t_in / t_sq_in, 3),
                nearest_gather_ms=t_gather, bytes=int(b), distance_sq_roofline_share=round(b / (t_sq * 1e-3) / ROOF, 4),
                nearest_roofline_share=round(b / (t_near * 1e-3) / ROOF, 4),
                kernels_distance_sq_ms_launches=kernels(lambda: g.distance_sq_device(out=dsq)),
                kernels_nearest_ms_launches=kernels(lambda: g.nearest_device(out=near)),
                kernels_nearest_gather_ms_launches=kernels(lambda: g.nearest_gather_device(vals, out=near)))


def mesh_case(name, vs, solid, reps):
    v, t = vx_scenes.scene(name)
    g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), np.float32(vs), solid=solid)
    return time_grid("%s vs=%g%s" % (name, vs, " solid" if solid else ""), g, reps)


def column_case(reps):
    X, Y, Z = 4, 4, 65536
    cells = np.random.default_rng(1).random((Z, Y, X)) < 2e-4
    g = voxhip.Grid.create(voxhip.GRID_BOOL, X, Y, Z, np.float32(1.0))
    words = solid_ref.pack(cells)

    class View:
        __cuda_array_interface__ = {"shape": (len(words),), "typestr": "<i4", "data": (g.bitmask_device_ptr(mutable=True), False), "version": 3,
                                    "strides": None}
    torch.as_tensor(View(), device="cuda").copy_(torch.from_numpy(words.view(np.int32)).cuda())
    torch.cuda.synchronize()
    g.refresh()
    return time_grid("long z columns 4 x 4 x 65536", g, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = [mesh_case("blob70k", 2.0 / 256, False, a.reps), mesh_case("blob70k", 2.0 / 256, True, a.reps),
           mesh_case("blob70k", 2.0 / 512, False, a.reps), mesh_case("blob70k", 2.0 / 512, True, a.reps),
           mesh_case("atrium262k", 32.0 / 512, False, a.reps), column_case(a.reps)]
    print(json.dumps(dict(tool="nearest_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, results=res)))


if __name__ == "__main__":
    main()
