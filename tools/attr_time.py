#!/usr/bin/env python3
"""Attribute shading (vx_render_set_shading(VX_RENDER_ATTRIBUTES)) timed by device events, one JSON line: a 1280x720 frame of the 32x32 field
of blob instances (smooth corner normals, spherical uvs into a 1024x1024 texture: vx_scenes.attr_blob_field) beside the atrium voxels at
512^3, as tools/instance_time.py's field_frame, in the default mode and in attribute mode (median over --frames), and the per-kernel times of
the shadow-ray and shading stages of both modes (vx_profile_*, summed over --frames frames).
   usage: attr_time.py [--frames 30]"""
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


def kernel_ms(f, reps):
    """per-kernel mean ms over reps calls of f, for the render stages"""
    voxhip.profile_reset()
    voxhip.profile_enable(True)
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    voxhip.profile_enable(False)
    return {name: round(ms / max(n, 1), 4) for name, (ms, n) in voxhip.profile_read().items() if "k_render_" in name}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    a = ap.parse_args()
    v, t = vx_scenes.scene("atrium262k")
    grid = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), np.float32(32.0 / 512))
    f = vx_scenes.attr_blob_field()
    mesh = voxhip.Mesh.from_arrays(f["verts"], f["tris"])
    mesh.set_attributes(f["normals"], f["uvs"])
    rec = np.zeros(1, voxhip.MATERIAL)
    rec["ambient"], rec["diffuse"], rec["specular"], rec["shininess"], rec["illum"] = 0.05, 0.9, 0.3, 32.0, 2
    mesh.set_materials(rec, np.zeros(mesh.num_triangles, np.int32))
    mesh.set_material_textures([0])
    mesh.set_texture(0, f["texture"])
    tl = voxhip.Tlas([mesh.bvh()], voxhip.instances(f["transforms"]))
    r = voxhip.Renderer.from_tlas(grid, tl, [mesh])
    W, H = 1280, 720
    vi, pi = vx_scenes.camera_matrices(**vx_scenes.INTERIOR_CAMERAS[0], aspect=W / H)
    cam = (vi, pi, W, H)
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    out = {"instances": len(f["transforms"]), "triangles_per_blob": int(mesh.num_triangles), "texture": list(f["texture"].shape[:2]), "size": [W, H]}
    for mode, flag in (("default", 0), ("attributes", voxhip.RENDER_ATTRIBUTES)):
        r.set_shading(flag)
        ms = median_ms(lambda: r.render(cam, out=img), a.frames)
        out[mode] = {"frame_ms": round(ms, 4), "kernels_ms": kernel_ms(lambda: r.render(cam, out=img), a.frames)}
    kind = torch.empty(W * H, dtype=torch.uint8, device="cuda")
    r.render(cam, out=img, kind=kind)
    torch.cuda.synchronize()
    k = kind.cpu().numpy()
    out["pixels_voxel"], out["pixels_triangle"] = int((k == 1).sum()), int((k == 2).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
