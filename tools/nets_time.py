#!/usr/bin/env python3
"""Surface nets (vx_grid_surface_smooth_device) timed by device events, one JSON line.  Per case: the median of --reps calls with 0 and with
8 iterations (lambda 0.5, mu -0.53: 16 steps), with normals, into preallocated device buffers; vx_grid_surface_device on the same grid in
the same session as the yardstick; one relax step alone (k_nets_relax's time per launch in a profiled 8-iteration call, vx_profile_*), the
bytes a step moves (per vertex: the six neighbour indices, 24; the own offset read, 12, which is also what the gathers of the neighbours'
offsets add up to when every offset is fetched once; the new offset, 12) and their share of an 8 TB/s roofline; and the per-kernel times of
one 8-iteration call.  Cases: surface_time.py's -- the blob at 256^3 and 512^3, surface and solid; the atrium at 512^3.
   usage: nets_time.py [--reps 10]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402
from surface_time import ROOF, kernels, median_ms  # noqa: E402

STEP_BYTES = 48  # per vertex and step


def time_grid(label, g, reps):
    X, Y, Z = g.describe()["dim"]
    nv, nt = g.surface_counts()
    xyz = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    nrm = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    tri = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    L = voxhip.lib()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()

    def blocky():
        voxhip._check(L.vx_grid_surface_device(g.h, xyz.data_ptr(), nv, tri.data_ptr(), nt, None, ctypes.byref(a), ctypes.byref(b)))

    def smooth(iterations):
        sp = voxhip.Smooth(iterations, 0.5, -0.53)

        def call():
            voxhip._check(L.vx_grid_surface_smooth_device(g.h, ctypes.byref(sp), xyz.data_ptr(), nv, tri.data_ptr(), nt, None, nrm.data_ptr(),
                                                          ctypes.byref(a), ctypes.byref(b)))
        return call

    t_blocky = median_ms(blocky, reps)
    t0 = median_ms(smooth(0), reps)
    t8 = median_ms(smooth(8), reps)
    k = kernels(smooth(8))
    relax = [v for name, v in k.items() if "k_nets_relax" in name]
    step_ms = round(relax[0][0] / relax[0][1], 5) if relax else None
    step_bytes = STEP_BYTES * nv
    return dict(case=label, dim=(X, Y, Z), vertices=nv, triangles=nt, surface_device_ms=t_blocky, smooth0_device_ms=t0, smooth8_device_ms=t8,
                relax_step_ms=step_ms, relax_step_bytes=step_bytes,
                relax_roofline_share=round(step_bytes / (step_ms * 1e-3) / ROOF, 4) if step_ms else None, kernels_ms_launches=k)


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
    print(json.dumps(dict(tool="nets_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, results=res)))


if __name__ == "__main__":
    main()
