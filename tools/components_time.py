#!/usr/bin/env python3
"""Connected components (vx_grid_components_device) timed by device events, one JSON line.  Per case and connectivity: the median of --reps
calls (the local, merge, flatten and label passes and the scan, into a preallocated label tensor, K on the device; no host wait), K, the
algorithmic bytes (the mask read by the local, merge, flatten and label passes: 4 x N/8; the parent written, read and rewritten for the
occupied cells: 3 x 4 x occupied; every label written once: 4 x N; the root words written, scanned and read: 3 x N/8), their share of an
8 TB/s roofline, and the per-kernel times of one call (vx_profile_*).  Cases at 512^3: the blob and the atrium (solid builds), a fully
occupied grid and a random mask at the percolation density of the connectivity (0.31 for 6, 0.10 for 26).
   usage: components_time.py [--reps 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402
from solid_ref import pack  # noqa: E402

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


def time_grid(label, g, connectivity, reps):
    X, Y, Z = g.describe()["dim"]
    n = X * Y * Z
    occ = g.describe()["occupied"]
    lab = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    kd = torch.empty(1, dtype=torch.int32, device="cuda")
    L = voxhip.lib()

    def call():
        voxhip._check(L.vx_grid_components_device(g.h, connectivity, lab.data_ptr(), n, kd.data_ptr()))

    t = median_ms(call, reps)
    nbytes = 4 * n / 8 + 3 * 4 * occ + 4 * n + 3 * n / 8
    return dict(case=label, connectivity=connectivity, dim=(X, Y, Z), occupied=occ, components=int(kd.item()), components_device_ms=t,
                bytes=int(nbytes), roofline_share=round(nbytes / (t * 1e-3) / ROOF, 4), kernels_ms_launches=kernels(call))


def mask_grid(cells):
    Z, Y, X = cells.shape
    g = voxhip.Grid.create(voxhip.GRID_BOOL, X, Y, Z, np.float32(1.0))
    words = np.ascontiguousarray(pack(cells)).view(np.int32)

    class View:
        __cuda_array_interface__ = {"shape": (len(words),), "typestr": "<i4", "data": (g.bitmask_device_ptr(mutable=True), False), "version": 3,
                                    "strides": None}
    torch.as_tensor(View(), device="cuda").copy_(torch.from_numpy(words).cuda())
    torch.cuda.synchronize()
    g.refresh()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    res = []
    for name, vs in (("blob70k", 2.0 / 512), ("atrium262k", 32.0 / 512)):
        v, t = vx_scenes.scene(name)
        g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), np.float32(vs), solid=True)
        for c in (6, 26):
            res.append(time_grid("%s vs=%g solid" % (name, vs), g, c, a.reps))
        del g
    g = mask_grid(np.ones((512, 512, 512), bool))
    for c in (6, 26):
        res.append(time_grid("full 512^3", g, c, a.reps))
    del g
    rng = np.random.default_rng(3)
    for c, p in ((6, 0.31), (26, 0.10)):
        g = mask_grid(rng.random((512, 512, 512), dtype=np.float32) < p)
        res.append(time_grid("random 512^3 p=%g" % p, g, c, a.reps))
        del g
    print(json.dumps(dict(tool="components_time", device=torch.cuda.get_device_name(0), roofline_bytes_per_s=ROOF, results=res)))


if __name__ == "__main__":
    main()
