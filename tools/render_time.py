#!/usr/bin/env python3
"""Device frame timings (vx_render_frame_device through voxhip.Renderer), one JSON line.  Scene: the atrium (BASELINE configs[2], 261k
triangles) voxelized at 512^3 as a Bool grid, with the atrium itself as the triangle model.  Workloads: the interior camera
vx_scenes.INTERIOR_CAMERAS[0] at 1280x720 and 3840x2160, and the reference camera (main.cpp:92) at 1280x720.  Per workload:
  frame_ms      median over --frames frames (after warm-up) of device events recorded around each frame on the scene's stream;
  kernels_ms    per-kernel mean ms per frame from the library's vx_profile_* events over the same number of frames;
  cli_host_ms   the CLI's host path (voxilizer --render --mesh, host staging + host shading) on the same scene and size: the host wall of
                that command minus the wall of the same command without --render / --mesh, median of --cli-reps runs (the difference also
                holds the mesh's OBJ read and BVH build, a few ms).
   usage: render_time.py [--frames 50] [--cli-reps 3] [--no-cli]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxhip  # noqa: E402
import vx_scenes  # noqa: E402

VS = 32.0 / 512


def frame_ms(r, cam, out, frames):
    for _ in range(5):
        r.render(cam, out=out)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
    for a, b in ev:
        a.record()
        r.render(cam, out=out)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def kernels_ms(r, cam, out, frames):
    torch.cuda.synchronize()
    voxhip.profile_select(None)
    voxhip.profile_reset()
    voxhip.profile_enable(True)
    for _ in range(frames):
        r.render(cam, out=out)
    torch.cuda.synchronize()
    voxhip.profile_enable(False)
    return {k: round(ms / frames, 4) for k, (ms, n) in sorted(voxhip.profile_read().items())}


def cli_ms(obj, W, H, reps):
    exe = os.path.join(PKG, "voxilizer")
    base = [exe, obj, "%.9g" % VS]

    def wall(extra):
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            times.append((time.perf_counter() - t0) * 1e3)
            if r.returncode != 0:
                raise RuntimeError(r.stdout)
        return float(np.median(times))

    ppm = os.path.join(os.path.dirname(obj), "host.ppm")
    return wall(["--render", ppm, "--size", "%dx%d" % (W, H), "--mesh", obj]) - wall([])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    if voxhip.device_count() < 1:
        raise SystemExit("render_time.py needs a HIP device")
    v, t = vx_scenes.scene("atrium262k")
    mesh = voxhip.Mesh.from_arrays(v, t)
    grid = voxhip.Grid.voxelize(mesh, np.float32(VS))
    bvh = mesh.bvh()
    r = voxhip.Renderer(grid, bvh, mesh)
    res = {"scene": "atrium262k@512^3 + atrium mesh", "frames": a.frames}
    tmp = tempfile.mkdtemp()
    obj = os.path.join(tmp, "atrium.obj")
    if not a.no_cli:
        vx_scenes.write_obj(obj, v, t)
    work = [("interior0_1280x720", vx_scenes.INTERIOR_CAMERAS[0], 1280, 720), ("interior0_3840x2160", vx_scenes.INTERIOR_CAMERAS[0], 3840, 2160),
            ("reference_1280x720", None, 1280, 720)]
    for name, cam_kw, W, H in work:
        vi, pi = vx_scenes.camera_matrices(**(cam_kw or {}), aspect=W / H)
        cam = (vi, pi, W, H)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        kind = torch.empty(W * H, dtype=torch.uint8, device="cuda")
        r.render(cam, out=out, kind=kind)
        torch.cuda.synchronize()
        k = kind.cpu().numpy()
        w = {"frame_ms": round(frame_ms(r, cam, out, a.frames), 4), "kernels_ms": kernels_ms(r, cam, out, a.frames),
             "voxel_px": int((k == 1).sum()), "triangle_px": int((k == 2).sum()), "miss_px": int((k == 0).sum())}
        w["fps"] = round(1000.0 / w["frame_ms"], 1)
        if not a.no_cli and cam_kw is None:   # the CLI renders from the reference camera only
            w["cli_host_ms"] = round(cli_ms(obj, W, H, a.cli_reps), 1)
        res[name] = w
        del out, kind
    if not a.no_cli:
        os.remove(obj)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
