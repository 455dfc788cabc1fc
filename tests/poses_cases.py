"""Bodies, transforms and non-finite variants of the pose-query tests (test_poses_cpu.py, test_gpu_poses.py)."""
import numpy as np

import field_cases as fc

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F)


def body(P, vs, seed, ball_cells=2.5, radius_cells=1.5):
    """P points in a ball of ball_cells cells around the body's origin, radii up to radius_cells cells -> f32[P, 3], f32[P]"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    pts = d * (rng.random((P, 1)) ** (1.0 / 3.0)) * ball_cells * float(vs)
    return pts.astype(F), (rng.random(P) * radius_cells * float(vs)).astype(F)


def rotations(N, seed):
    """N uniformly random rotation matrices (unit quaternions) -> f64[N, 3, 3]"""
    q = np.random.default_rng(seed).normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(N, 3, 3)


def transforms(dims, org, vs, N, seed, grow_cells=2.0):
    """N random rotations, translated into the grid's box grown by grow_cells cells -> f32[N, 12], row-major 3 x 4"""
    R = rotations(N, seed)
    t = fc.random_points(dims, org, vs, N, seed + 1000, grow_cells=grow_cells)
    return np.concatenate([R, t[:, :, None].astype(np.float64)], axis=2).reshape(N, 12).astype(F)


def nonfinite_variants(pts, radii, xf):
    """Copies of (points, radii, transforms) with non-finite entries, each named: single points, single radii, single transform entries, a
    pose whose every point is skipped, and overflowing transforms.  Needs at least 8 poses and (for the point and radius edits) uses
    indices modulo the body's size."""
    P, N = len(pts), len(xf)
    out = []
    if P:
        p = pts.copy()
        p[0 % P, 0], p[(P // 2) % P, 1], p[P - 1, 2] = np.nan, np.inf, -np.inf
        out.append(("points", p, radii, xf))
        r = radii.copy()
        r[0 % P], r[(P // 3) % P], r[P - 1] = np.nan, np.inf, -np.inf
        out.append(("radii", pts, r, xf))
    m = xf.copy()
    m[0, 0], m[1, 5], m[2, 10] = np.nan, np.inf, -np.inf          # rotation entries: the points with a zero coordinate there stay
    m[3, 3], m[4, 7], m[5, 11] = np.inf, -np.inf, np.nan          # translations: every point of the pose is skipped
    m[6, :] = np.nan
    out.append(("transform entries", pts, radii, m))
    m = xf.copy()
    m[0, :] = F(3e38)                                             # products and sums overflow: inf, and inf - inf
    m[1, 0:3] = F(3e38)
    m[2, 3] = F(3e38)
    m[3, 4:8] = F(-3e38)
    m[N - 1, 8:11] = (F(3e38), F(-3e38), F(3e38))
    out.append(("overflowing transforms", pts, radii, m))
    return out
