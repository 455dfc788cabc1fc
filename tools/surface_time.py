#!/usr/bin/env python3
"""Surface mesh (vx_grid_surface_device) timed by device events, one JSON line.  Per case: the median of --reps calls (the counting pass, both
scans, the host's wait for the two counts and the emission, into preallocated device buffers), V and T, the algorithmic bytes (the mask read
by the counting and the emission pass: 2 x N/8; the corner words written, scanned and read twice: 4 x L/8 for L lattice points; the triangle
counts and both prefixes: 3 x 4 x (nwords + L/32); the outputs: 12 V + 12 T), their share of an 8 TB/s roofline, and the per-kernel times
of one call (vx_profile_*).  Cases: the blob at 256^3 and 512^3, surface and solid; the atrium at 512^3.
   usage: surface_time.py [--reps 10]"""
import argparse
import ctypes
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
    return {name: [round(ms, 4), n] for name, (ms, n) in voxhip.profile_read().items()}


def time_grid(label, g, reps):
    X, Y, Z = g.describe()["dim"]
    nv, nt = g.surface_counts()
    xyz = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    tri = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    L = voxhip.lib()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()

    def call():
        voxhip._check(L.vx_grid_surface_device(g.h, xyz.data_ptr(), nv, tri.data_ptr(), nt, None, ctypes.byref(a), ctypes.byref(b)))

    t = median_ms(call, reps)
    n = X * Y * Z
    lat = (X + 1) * (Y + 1) * (Z + 1)
    nbytes = 2 * n / 8 + 4 * lat / 8 + 3 * 4 * ((n + 31) // 32 + (lat + 31) // 32) + 12 * nv + 12 * nt
    return dict(case=label, dim=(X, Y, Z), occupied=g.describe()["occupied"], vertices=nv, triangles=nt, surface_device_ms=t,
                bytes=int(nbytes), roofline_share=round(nbytes / (t * 1e-3) / ROOF, 4), kernels_ms_launches=kernels(call))


def mesh_case(name, vs, solid, reps):
    v, t = vx_scenes.scene(name)
    g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), np.float32(vs), solid=solid)
    return time_grid("%s vs=%g%s" % (name, vs, " solid" if solid else ""), g, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = [mesh_case("blob70k", 2.0 / 256, False, a.reps), mesh_case("blob70k", 2.0 / 256, True, a.reps),
           mesh_case("blob70k", 2.0 / 512, False, a.reps), mesh_case("blob70k", 2.0 / 512, True, a.reps),
           mesh_case("atrium262k", 32.0 / 512, False, a.reps)]
    print(json.dumps(dict(tool="surface_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, results=res)))


if __name__ == "__main__":
    main()
