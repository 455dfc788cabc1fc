#!/usr/bin/env python3
"""Distance fields (vx_grid_distance_sq_device, vx_grid_sdf_device) timed by device events, one JSON line.  Per case: the median of --reps
calls of the squared field (D_out) and of the signed field, the algorithmic bytes of the passes built (x pass: the mask in, N x 4 B out; y and
z passes: N x 4 B in and out, in place; the signed field's column passes also read the mask: N/8 + 4N + 2 x 8N, and 2 x N/8 more for the
signed field), their share of an 8 TB/s roofline, and the per-kernel times of one call of each (vx_profile_*).  The envelopes' stacks
(8 B per entry pushed and read back, [k][column] in global scratch) are not in the algorithmic bytes: they depend on the data.
Cases: the blob at 256^3 and 512^3, surface and solid; the atrium at 512^3; a 4 x 4 x 65536 mask with one cell in 5000 occupied.
   usage: distance_time.py [--reps 10]"""
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
    return {name: [round(ms, 4), n] for name, (ms, n) in voxhip.profile_read().items() if "dist" in name}


def time_grid(label, g, reps):
    X, Y, Z = g.describe()["dim"]
    n = X * Y * Z
    dsq = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    sdf = torch.empty((Z, Y, X), dtype=torch.float32, device="cuda")
    t_sq = median_ms(lambda: g.distance_sq_device(out=dsq), reps)
    t_sdf = median_ms(lambda: g.sdf_device(out=sdf), reps)
    b_sq = n / 8 + 4 * n + 2 * 8 * n
    b_sdf = b_sq + 2 * n / 8
    return dict(case=label, dim=(X, Y, Z), occupied=g.describe()["occupied"], distance_sq_ms=t_sq, sdf_ms=t_sdf,
                distance_sq_bytes=int(b_sq), sdf_bytes=int(b_sdf),
                distance_sq_roofline_share=round(b_sq / (t_sq * 1e-3) / ROOF, 4), sdf_roofline_share=round(b_sdf / (t_sdf * 1e-3) / ROOF, 4),
                kernels_distance_sq_ms_launches=kernels(lambda: g.distance_sq_device(out=dsq)),
                kernels_sdf_ms_launches=kernels(lambda: g.sdf_device(out=sdf)))


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
    print(json.dumps(dict(tool="distance_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, results=res)))


if __name__ == "__main__":
    main()
