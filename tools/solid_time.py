#!/usr/bin/env python3
"""Solid voxelization (VX_VOXELIZE_SOLID) timed by device events, one JSON line.  Per case: the median of a surface build and of a solid build
on one handle (the difference is what the fill adds to a build: seed, rounds, finish, the scan over H and the host's batch waits), the number
of flood-fill rounds (the quiet one included), |H|, and the per-kernel times of the fill's kernels in one solid build (vx_profile_*; kernels of
rounds after the quiet one exit at once and are counted too).  Cases: the blob at 256^3 and 512^3, the atrium at 512^3 (open at the front: the
exterior fills most of the grid and winds through the hall), and the 3-D spiral maze (vx_scenes.spiral_maze) written into a Bool grid through
vx_grid_bitmask_device_mut and filled by vx_grid_fill_interior, and a 37 x 9 x N block crossed by a channel along z (the column scans over
thousands of chunks per column).
   usage: solid_time.py [--reps 10] [--maze 256] [--channel 200000]"""
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


def median_ms(f, reps, before=None):
    for _ in range(2):
        if before:
            before()
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if before:
            before()
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
    return {name: [round(ms, 4), n] for name, (ms, n) in voxhip.profile_read().items() if "solid" in name}


def build_case(name, vs, reps):
    v, t = vx_scenes.scene(name)
    mesh = voxhip.Mesh.from_arrays(v, t)
    g = voxhip.Grid.voxelize(mesh, np.float32(vs))
    surface = median_ms(lambda: g.revoxelize(mesh, np.float32(vs)), reps)
    solid = median_ms(lambda: g.revoxelize(mesh, np.float32(vs), solid=True), reps)
    k = kernels(lambda: g.revoxelize(mesh, np.float32(vs), solid=True))
    return dict(case="%s vs=%g" % (name, vs), dim=g.describe()["dim"], surface_build_ms=surface, solid_build_ms=solid,
                fill_ms=round(solid - surface, 4), rounds=g.fill_rounds(), interior=g.interior(), kernels_ms_launches=k)


def channel_cells(L):
    """37 x 9 x L: a solid block with a one-cell channel open at z = 0 running almost to z = L and a closed cavity beside it"""
    cells = np.ones((L, 9, 37), bool)
    cells[0:L - 10, 4, 18] = False
    cells[5:L - 5, 3:6, 8:11] = False
    return cells


def mask_case(label, cells, reps):
    Z, Y, X = cells.shape
    words = solid_ref.pack(cells)
    g = voxhip.Grid.create(voxhip.GRID_BOOL, X, Y, Z, np.float32(1.0))
    src = torch.from_numpy(words.view(np.int32)).cuda()

    class View:
        __cuda_array_interface__ = {"shape": (len(words),), "typestr": "<i4", "data": (g.bitmask_device_ptr(mutable=True), False), "version": 3,
                                    "strides": None}
    dst = torch.as_tensor(View(), device="cuda")

    def restore():
        dst.copy_(src)
        torch.cuda.synchronize()
        g.bitmask_device_ptr(mutable=True)
    fill = median_ms(lambda: g.fill_interior(), reps, before=restore)
    restore()
    k = kernels(lambda: g.fill_interior())
    return dict(case=label + " (fill_interior, incl. the refresh)", dim=(X, Y, Z), fill_interior_ms=fill, rounds=g.fill_rounds(),
                interior=g.interior(), kernels_ms_launches=k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maze", type=int, default=256)
    ap.add_argument("--channel", type=int, default=200_000, help="z length of the channel mask (37 x 9 x N cells)")
    a = ap.parse_args()
    res = [build_case("blob70k", 2.0 / 256, a.reps), build_case("blob70k", 2.0 / 512, a.reps), build_case("atrium262k", 32.0 / 512, a.reps),
           mask_case("spiral maze %d^3" % a.maze, vx_scenes.spiral_maze(a.maze), a.reps),
           mask_case("long z channel", channel_cells(a.channel), a.reps)]
    print(json.dumps(dict(tool="solid_time", device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
