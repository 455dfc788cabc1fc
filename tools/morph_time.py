#!/usr/bin/env python3
"""Morphology (vx_grid_morph_device) timed by device events, one JSON line.  Per grid (the blob's surface at 256^3 and 512^3), operation
(DILATE, CLOSE) and squared radius: the median of --reps calls and the per-kernel times of one call (vx_profile_*), with the path the library
took (bit-level kernel or distance fields) read off the kernels it launched.
The crossover vx_morph_bit_radius() is a build constant: to time BOTH paths at every radius, build two more libraries with
VOXHIP_EXTRA_FLAGS=-DVX_MORPH_BIT_RADIUS=0 (distance fields from r2 = 1 on) and =32 (bit-level up to R = 32) and pass each with --lib.
   usage: morph_time.py [--reps 10] [--lib PATH/libvoxhip.so] [--sizes 256,512]"""
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

R2S = [1, 3, 9, 25, 64, 144, 256, 1024]


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
    return {name: [round(ms, 4), n] for name, (ms, n) in voxhip.profile_read().items() if "morph" in name or "dist" in name}


def time_grid(size, reps):
    v, t = vx_scenes.scene("blob70k")
    g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), np.float32(2.0 / size))
    d = g.describe()
    out = torch.empty(d["num_words"], dtype=torch.int32, device="cuda")
    rows = []
    for op, name in ((voxhip.MORPH_DILATE, "dilate"), (voxhip.MORPH_CLOSE, "close")):
        for r2 in R2S:
            ms = median_ms(lambda: g.morph_mask_device(op, r2, out=out), reps)
            ks = kernels(lambda: g.morph_mask_device(op, r2, out=out))
            path = "distance" if any("k_dist_col" in k for k in ks) else "bit"
            rows.append(dict(op=name, r2=r2, ms=ms, path=path, kernels_ms_launches=ks))
            print("%s %d^3 %s r2=%d: %.4f ms (%s)" % ("blob", size, name, r2, ms, path), file=sys.stderr, flush=True)
    return dict(case="blob70k vs=2/%d" % size, dim=d["dim"], occupied=d["occupied"], rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--sizes", default="256,512")
    a = ap.parse_args()
    if a.lib:
        voxhip.LIB_PATH = os.path.abspath(a.lib)
    res = [time_grid(int(s), a.reps) for s in a.sizes.split(",")]
    print(json.dumps(dict(tool="morph_time", device=torch.cuda.get_device_name(0), bit_radius=voxhip.morph_bit_radius(), results=res)))


if __name__ == "__main__":
    main()
