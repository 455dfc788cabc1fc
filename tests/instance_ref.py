"""Numpy restatement of the instanced-scene contract of include/voxhip.h (vx_tlas_*): the pinned float64 world-to-object inverse, the
float32 object-space rays, and the brute force over every active (instance, triangle) pair -- a per-instance mesh_ref.closest / any_hit
followed by the lexicographic minimum of (t, instance, prim)."""
import numpy as np

import mesh_ref

MISS = np.uint32(0xFFFFFFFF)
INSTANCE = np.dtype([("transform", np.float32, (12,)), ("blas", np.uint32), ("mask", np.uint32)])


def make_instances(transforms, blas=None, mask=None):
    tr = np.asarray(transforms, np.float32).reshape(-1, 12)
    out = np.zeros(tr.shape[0], INSTANCE)
    out["transform"] = tr
    out["blas"] = 0 if blas is None else np.asarray(blas, np.uint32)
    out["mask"] = 0xFF if mask is None else np.asarray(mask, np.uint32)
    return out


def inverse(transforms):
    """-> (W float32[n, 12], det float64[n]): the header's adjugate formula, operation for operation in float64, then rounded."""
    m = np.asarray(transforms, np.float32).reshape(-1, 12).astype(np.float64)
    a0, a1, a2, t0, a4, a5, a6, t1, a8, a9, a10, t2 = (m[:, k] for k in range(12))
    c = [a5 * a10 - a6 * a9, a6 * a8 - a4 * a10, a4 * a9 - a5 * a8,
         a2 * a9 - a1 * a10, a0 * a10 - a2 * a8, a1 * a8 - a0 * a9,
         a1 * a6 - a2 * a5, a2 * a4 - a0 * a6, a0 * a5 - a1 * a4]
    with np.errstate(all="ignore"):
        det = (a0 * c[0] + a1 * c[1]) + a2 * c[2]
        w = np.zeros((m.shape[0], 12), np.float32)
        for r in range(3):
            i0, i1, i2 = c[0 * 3 + r] / det, c[1 * 3 + r] / det, c[2 * 3 + r] / det
            tr = -((i0 * t0 + i1 * t1) + i2 * t2)
            w[:, 4 * r], w[:, 4 * r + 1], w[:, 4 * r + 2], w[:, 4 * r + 3] = (x.astype(np.float32) for x in (i0, i1, i2, tr))
    return w, det


def active(inst, ntri):
    """ntri[b] = the triangle count of BLAS b"""
    w, det = inverse(inst["transform"])
    nb = len(ntri)
    ok = (inst["mask"] != 0) & (inst["blas"] < nb) & np.isfinite(det) & (det != 0) & np.isfinite(w).all(axis=1)
    for i in np.nonzero(ok)[0]:
        ok[i] = ntri[int(inst["blas"][i])] > 0
    return ok


def object_rays(w, rays):
    """o' = ((w0*ox + w1*oy) + w2*oz) + w3, d' = (w0*dx + w1*dy) + w2*dz per row, float32"""
    r = np.asarray(rays, np.float32).reshape(-1, 6)
    w = np.asarray(w, np.float32).reshape(12)
    out = np.empty_like(r)
    with np.errstate(all="ignore"):
        for k in range(3):
            w0, w1, w2, w3 = w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]
            out[:, k] = ((w0 * r[:, 0] + w1 * r[:, 1]) + w2 * r[:, 2]) + w3
            out[:, 3 + k] = (w0 * r[:, 3] + w1 * r[:, 4]) + w2 * r[:, 5]
    return out


def closest(meshes, inst, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    """meshes[b] = (verts, tris) of BLAS b -> (t, instance, prim, bary) of the lexicographically smallest (t, instance, prim)."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    t = np.full(n, -1.0, np.float32)
    ii = np.full(n, MISS, np.uint32)
    pp = np.full(n, MISS, np.uint32)
    bb = np.zeros((n, 2), np.float32)
    w, _ = inverse(inst["transform"])
    act = active(inst, [len(np.asarray(tr).reshape(-1, 3)) for _, tr in meshes])
    for i in np.nonzero(act)[0]:
        v, tr = meshes[int(inst["blas"][i])]
        ti, pi, bi = mesh_ref.closest(v, tr, object_rays(w[i], rays), tmin, tmax, tmax_per_ray)
        better = (ti > 0) & ((t < 0) | (ti < t))   # instances in increasing order: a tie keeps the lower instance
        t[better], ii[better], pp[better], bb[better] = ti[better], np.uint32(i), pi[better], bi[better]
    return t, ii, pp, bb


def any_hit(meshes, inst, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros(rays.shape[0], np.uint8)
    w, _ = inverse(inst["transform"])
    act = active(inst, [len(np.asarray(tr).reshape(-1, 3)) for _, tr in meshes])
    for i in np.nonzero(act)[0]:
        v, tr = meshes[int(inst["blas"][i])]
        out |= mesh_ref.any_hit(v, tr, object_rays(w[i], rays), tmin, tmax, tmax_per_ray)
    return out


def world_vertices(transform, p):
    """M*v per row in the pinned association ((m0*x + m1*y) + m2*z) + m3, float32"""
    m = np.asarray(transform, np.float32).reshape(12)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    return np.stack([((m[4 * k] * p[:, 0] + m[4 * k + 1] * p[:, 1]) + m[4 * k + 2] * p[:, 2]) + m[4 * k + 3] for k in range(3)], axis=1)


def world_hit_points(meshes, inst, instance, prim, bary):
    """M * ((p0*b0 + p1*b1) + p2*b2), b0 = (1 - b1) - b2: the triangle hit point the frame's shading uses"""
    out = np.zeros((len(instance), 3), np.float32)
    for r in np.nonzero(instance != MISS)[0]:
        i = int(instance[r])
        v, tr = meshes[int(inst["blas"][i])]
        tri = np.asarray(tr).reshape(-1, 3)[int(prim[r])]
        p = np.asarray(v, np.float32).reshape(-1, 3)[tri]
        b1, b2 = np.float32(bary[r, 0]), np.float32(bary[r, 1])
        b0 = np.float32(1.0) - b1 - b2
        out[r] = world_vertices(inst["transform"][i], ((p[0] * b0 + p[1] * b1) + p[2] * b2)[None])[0]
    return out


def world_normals(meshes, inst, instance, prim):
    """the unit geometric normal of the world-space triangle (cross(e1, e2) / |.|, not flipped); zeros on a miss"""
    out = np.zeros((len(instance), 3), np.float32)
    for r in np.nonzero(instance != MISS)[0]:
        i = int(instance[r])
        v, tr = meshes[int(inst["blas"][i])]
        tri = np.asarray(tr).reshape(-1, 3)[int(prim[r])]
        p = world_vertices(inst["transform"][i], np.asarray(v, np.float32).reshape(-1, 3)[tri])
        e1, e2 = p[1] - p[0], p[2] - p[0]
        c = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        out[r] = (c / np.linalg.norm(c)).astype(np.float32)
    return out


def transform(rot=np.eye(3), scale=(1.0, 1.0, 1.0), shear=0.0, offset=(0.0, 0.0, 0.0)):
    """row-major 3x4 object-to-world: rot @ shear @ diag(scale), then offset"""
    sh = np.eye(3)
    sh[0, 1] = shear
    a = np.asarray(rot, np.float64) @ sh @ np.diag(np.asarray(scale, np.float64))
    out = np.zeros((3, 4), np.float64)
    out[:, :3] = a
    out[:, 3] = offset
    return out.reshape(12).astype(np.float32)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q
