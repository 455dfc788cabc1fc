#!/usr/bin/env python3
"""Instanced scenes (vx_tlas_*) timed by device events, one JSON line:
  identity      k_tlas_trace with one identity instance of the atrium mesh (261k triangles) against k_bvh_trace on the same 1M random rays;
  update_ms     vx_tlas_update_device of 1k / 100k / 1M instances of a 5.9k-triangle blob (median of --reps), and the built height;
  field_frame   frame time (median over --frames) at 1280x720 of a 32x32 field of blob instances beside the atrium voxels at 512^3, with a
                vx_tlas_update_device before every frame and without.
   usage: instance_time.py [--frames 30] [--reps 10]"""
import argparse
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


def median_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        f()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def scaled(n, s, lo, hi, seed=1):
    rng = np.random.default_rng(seed)
    tr = np.zeros((n, 12), np.float32)
    tr[:, 0] = tr[:, 5] = tr[:, 10] = s
    tr[:, [3, 7, 11]] = rng.uniform(lo, hi, (n, 3))
    return voxhip.instances(tr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    out = {}
    v, t = vx_scenes.scene("atrium262k")
    mesh = voxhip.Mesh.from_arrays(v, t)
    bvh = mesh.bvh()
    ident = np.zeros(12, np.float32)
    ident[[0, 5, 10]] = 1
    tl = voxhip.Tlas([bvh], voxhip.instances([ident]))
    n = 1_000_000
    rays = torch.from_numpy(vx_scenes.random_rays(n, v.min(0), v.max(0), seed=11)).cuda()
    tt = torch.empty(n, device="cuda")
    pp = torch.empty(n, dtype=torch.int32, device="cuda")
    kb = median_ms(lambda: bvh.trace_device(rays.data_ptr(), n, tt.data_ptr(), pp.data_ptr()), a.reps)
    kt = median_ms(lambda: tl.trace_device(rays.data_ptr(), n, tt.data_ptr(), pp.data_ptr()), a.reps)
    out["identity"] = {"rays": n, "k_bvh_trace_ms": round(kb, 4), "k_tlas_trace_ms": round(kt, 4), "ratio": round(kt / kb, 3)}
    bv, bt = vx_scenes.blob(nlon=60, nlat=50)
    bm = voxhip.Mesh.from_arrays(bv, bt)
    bb = bm.bvh()
    out["update_ms"] = {}
    for m in (1000, 100_000, 1_000_000):
        inst = scaled(m, 0.1, -100, 100)
        T = voxhip.Tlas([bb], inst)
        dev = torch.from_numpy(inst.view(np.uint8).copy()).cuda()
        out["update_ms"][str(m)] = {"ms": round(median_ms(lambda: T.update(device_ptr=dev, count=m), a.reps), 4), "height": T.height()}
    grid = voxhip.Grid.voxelize(mesh, np.float32(32.0 / 512))
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    tr = np.zeros((1024, 12), np.float32)
    tr[:, 0] = tr[:, 5] = tr[:, 10] = 0.3
    tr[:, 3] = -12 + g[:, 0] * 0.75
    tr[:, 7] = 1.0
    tr[:, 11] = -12 + g[:, 1] * 0.75
    inst = voxhip.instances(tr)
    T = voxhip.Tlas([bb], inst)
    dev = torch.from_numpy(inst.view(np.uint8).copy()).cuda()
    r = voxhip.Renderer.from_tlas(grid, T, [bm])
    W, H = 1280, 720
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=W / H)
    cam = (vi, pi, W, H)
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    f0 = median_ms(lambda: r.render(cam, out=img), a.frames)

    def upd_frame():
        T.update(device_ptr=dev, count=1024)
        r.render(cam, out=img)
    f1 = median_ms(upd_frame, a.frames)
    kind = torch.empty(W * H, dtype=torch.uint8, device="cuda")
    r.render(cam, out=img, kind=kind)
    torch.cuda.synchronize()
    k = kind.cpu().numpy()
    out["field_frame"] = {"instances": 1024, "size": [W, H], "frame_ms": round(f0, 4), "update_and_frame_ms": round(f1, 4), "tlas_height": T.height(),
                          "pixels_voxel": int((k == 1).sum()), "pixels_triangle": int((k == 2).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
