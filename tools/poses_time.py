#!/usr/bin/env python3
"""Pose queries (vx_field_poses_device) timed on the atrium at 512^3, solid; one JSON line.  Medians (with the smallest and largest) of --reps
calls by device events, after warm-up, into preallocated tensors.  Two regimes:
  spheres   32 spheres in a ball of 2.5 cells x 10^6 poses (random rotations, translated uniformly into the grid's box)
  shell     10^5 points taken from the grid's own surface cells, in random order, x 100 poses (random rotations about the box's centre,
            shifted by up to 8 cells); shell_sorted: the same points and poses with the points in the grid's cell order, so that a
            workgroup's 256 points are neighbours
Beside each, what a caller did before the fused query, in the same run and reported in its three parts: a torch transform of the N P
points, Field.sample_device (value only) on them, and a torch segmented amin and count of value - radius.
   usage: poses_time.py [--reps 10]"""
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

F = np.float32


def timed(f, reps):
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
    return dict(ms=round(float(np.median(out)), 4), min_ms=round(float(np.min(out)), 4), max_ms=round(float(np.max(out)), 4))


def rotations(n, rng):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def regime(field, label, pts, radii, R, t, margin, reps):
    P, N = len(pts), len(R)
    xf = np.concatenate([R, t[:, :, None]], axis=2).reshape(N, 12).astype(F)
    d_p, d_r, d_x = torch.from_numpy(pts).cuda(), torch.from_numpy(radii).cuda(), torch.from_numpy(xf).cuda()
    d_c = torch.empty(N, dtype=torch.float32, device="cuda")
    d_i = torch.empty(N, dtype=torch.int32, device="cuda")
    d_n = torch.empty(N, dtype=torch.int32, device="cuda")
    d_q = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    d_g = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    out = dict(regime=label, points=P, poses=N, point_poses=N * P)

    def per(r):
        r["ns_per_point_pose"] = round(r["ms"] * 1e6 / (N * P), 5)
        return r
    out["fused"] = per(timed(lambda: field.poses_device(d_p.data_ptr(), P, d_x.data_ptr(), N, radii_ptr=d_r.data_ptr(), margin=margin,
                                                        clearance=d_c.data_ptr(), point=d_i.data_ptr(), count=d_n.data_ptr()), reps))
    out["fused_all_outputs"] = per(timed(lambda: field.poses_device(d_p.data_ptr(), P, d_x.data_ptr(), N, radii_ptr=d_r.data_ptr(), margin=margin,
                                                                    clearance=d_c.data_ptr(), point=d_i.data_ptr(), count=d_n.data_ptr(),
                                                                    position=d_q.data_ptr(), gradient=d_g.data_ptr()), reps))
    torch.cuda.synchronize()
    fused_c, fused_n = d_c.clone(), d_n.clone()
    # the caller's own path
    Rt = d_x.view(N, 3, 4)[:, :, :3].transpose(1, 2).contiguous()
    tt = d_x.view(N, 3, 4)[:, :, 3].contiguous()
    q = torch.empty((N, P, 3), dtype=torch.float32, device="cuda")
    v = torch.empty(N * P, dtype=torch.float32, device="cuda")

    def transform():
        torch.matmul(d_p.unsqueeze(0), Rt, out=q)
        q.add_(tt.unsqueeze(1))

    def reduce():
        g = v.view(N, P) - d_r
        return g.amin(dim=1), (g <= margin).sum(dim=1)
    out["baseline_transform"] = per(timed(transform, reps))
    out["baseline_sample_device"] = per(timed(lambda: field.sample_device(q.data_ptr(), N * P, v.data_ptr()), reps))
    out["baseline_amin_count"] = per(timed(reduce, reps))
    out["baseline_total_ms"] = round(sum(out[k]["ms"] for k in ("baseline_transform", "baseline_sample_device", "baseline_amin_count")), 4)
    c, n = reduce()
    torch.cuda.synchronize()
    out["colliding_share"] = round(float((fused_n > 0).float().mean().item()), 4)
    # (torch's transform may fuse and reorder, so the two agree to rounding, not to the bit)
    out["largest_clearance_difference"] = float((c - fused_c).abs().max().item())
    out["count_mismatches"] = int((n.to(torch.int32) != fused_n).sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    v, t = vx_scenes.atrium()
    vs = F(32.0 / 512)
    g = voxhip.Grid.voxelize(voxhip.Mesh.from_arrays(v, t), vs, solid=True)
    d = g.describe()
    X, Y, Z = d["dim"]
    field = g.field()
    res = dict(tool="poses_time", device=torch.cuda.get_device_name(0), scene="atrium solid", dim=(X, Y, Z), occupied=d["occupied"], reps=a.reps)
    rng = np.random.default_rng(1)
    lo = np.asarray(d["origin"], dtype=np.float64)
    hi = lo + np.array([X, Y, Z]) * float(vs)
    # 32 spheres, 10^6 poses
    dirs = rng.normal(size=(32, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = (dirs * rng.random((32, 1)) ** (1 / 3) * 2.5 * float(vs)).astype(F)
    radii = (rng.random(32) * 1.5 * float(vs)).astype(F)
    N = 1_000_000
    res["spheres"] = regime(field, "32 spheres x 1e6 poses", pts, radii, rotations(N, rng), rng.random((N, 3)) * (hi - lo) + lo, 0.0, a.reps)
    # 10^5 points of the grid's own surface cells (occupied, with an empty cell one step away: value -vs), 100 poses about the box's centre
    sdf = torch.empty((Z, Y, X), dtype=torch.float32, device="cuda")
    g.sdf_device(out=sdf)
    cells = torch.nonzero((sdf < 0) & (sdf >= -float(vs))).cpu().numpy()
    del sdf
    available = len(cells)
    cells = cells[rng.permutation(available)[:100_000]]
    centre = (lo + hi) / 2
    pts = (lo + (cells[:, ::-1] + 0.5) * float(vs) - centre).astype(F)
    N = 100
    res["shell"] = regime(field, "1e5 surface points x 100 poses", pts, np.zeros(len(pts), dtype=F), rotations(N, rng),
                          centre + (rng.random((N, 3)) * 2 - 1) * 8 * float(vs), float(vs), a.reps)
    res["shell"]["surface_cells_available"] = int(available)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    rng = np.random.default_rng(2)
    rot = rotations(N, rng)
    shift = centre + (rng.random((N, 3)) * 2 - 1) * 8 * float(vs)
    res["shell_sorted"] = regime(field, "the same 1e5 points in cell order x 100 poses", pts[order], np.zeros(len(pts), dtype=F), rot, shift, float(vs), a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
