"""Numpy restatement of the triangle ray contract of include/voxhip.h (vx_bvh_trace*): Moeller-Trumbore over ALL triangles, strictly in
float32, in the pinned order of operations.  A helper for the tests, not a test itself.

    e1 = v1 - v0;  e2 = v2 - v0;  p = cross(d, e2);  det = dot(e1, p);  inv = 1 / det;  s = o - v0;  u = dot(s, p) * inv
    q = cross(s, e1);  v = dot(d, q) * inv;  t = dot(e2, q) * inv
    accepted iff u >= 0 and u <= 1 and v >= 0 and u + v <= 1 and t > 0 and t >= tmin and t <= tmax

closest():  t = the minimum accepted t (-1 on a miss), prim = the smallest triangle index reaching it (0xFFFFFFFF), bary = its (u, v).
any_hit():  1 iff some triangle is accepted.
"""
import numpy as np

MISS = np.uint32(0xFFFFFFFF)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _tris(verts, tris):
    v = np.asarray(verts, np.float32)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    v0, v1, v2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1 = tuple((v1[:, a] - v0[:, a])[None, :] for a in range(3))
    e2 = tuple((v2[:, a] - v0[:, a])[None, :] for a in range(3))
    return tuple(v0[:, a][None, :] for a in range(3)), e1, e2


def _mt(tri, rays, tmin, tmax):
    """(accepted, t, u, v) of every (ray, triangle) pair of the chunk, float32."""
    v0, e1, e2 = tri
    o = tuple(rays[:, a][:, None] for a in range(3))
    d = tuple(rays[:, 3 + a][:, None] for a in range(3))
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv = np.float32(1.0) / det
        s = tuple(o[a] - v0[a] for a in range(3))
        u = _dot(s, p) * inv
        q = _cross(s, e1)
        v = _dot(d, q) * inv
        t = _dot(e2, q) * inv
        acc = (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t >= tmin) & (t <= tmax)
    return acc, t, u, v


def _chunks(nrays, ntri, budget=1 << 22):
    c = max(1, budget // max(ntri, 1))
    for i in range(0, nrays, c):
        yield i, min(nrays, i + c)


def _bounds(rays, tmin, tmax, tmax_per_ray, i, j):
    tm = np.float32(tmax) if tmax_per_ray is None else np.asarray(tmax_per_ray, np.float32)[i:j][:, None]
    return np.float32(tmin), tm


def closest(verts, tris, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    """-> (t float32[n], prim uint32[n], bary float32[n, 2])"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    t_out = np.full(n, -1.0, np.float32)
    p_out = np.full(n, MISS, np.uint32)
    b_out = np.zeros((n, 2), np.float32)
    nt = int(np.asarray(tris).reshape(-1, 3).shape[0])
    if nt == 0 or n == 0:
        return t_out, p_out, b_out
    tri = _tris(verts, tris)
    for i, j in _chunks(n, nt):
        lo, hi = _bounds(rays, tmin, tmax, tmax_per_ray, i, j)
        acc, t, u, v = _mt(tri, rays[i:j], lo, hi)
        hit = acc.any(axis=1)
        tt = np.where(acc, t, np.float32(np.inf)).min(axis=1)
        k = np.argmax(acc & (t == tt[:, None]), axis=1)       # the first (smallest) index reaching the minimum
        rows = np.arange(j - i)
        t_out[i:j] = np.where(hit, tt, np.float32(-1.0))
        p_out[i:j] = np.where(hit, k.astype(np.uint32), MISS)
        b_out[i:j, 0] = np.where(hit, u[rows, k], np.float32(0))
        b_out[i:j, 1] = np.where(hit, v[rows, k], np.float32(0))
    return t_out, p_out, b_out


def any_hit(verts, tris, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    """-> uint8[n]: 1 iff some triangle is accepted"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    out = np.zeros(n, np.uint8)
    nt = int(np.asarray(tris).reshape(-1, 3).shape[0])
    if nt == 0 or n == 0:
        return out
    tri = _tris(verts, tris)
    for i, j in _chunks(n, nt):
        lo, hi = _bounds(rays, tmin, tmax, tmax_per_ray, i, j)
        out[i:j] = _mt(tri, rays[i:j], lo, hi)[0].any(axis=1)
    return out


def normals(verts, tris, prim):
    """The unit geometric normal cross(e1, e2) / |.| of every prim (zeros for misses), float32."""
    prim = np.asarray(prim, np.uint32)
    out = np.zeros((prim.size, 3), np.float32)
    h = prim != MISS
    if not h.any():
        return out
    v = np.asarray(verts, np.float32)
    t = np.asarray(tris, np.int64).reshape(-1, 3)[prim[h].astype(np.int64)]
    v0, v1, v2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1 = tuple(v1[:, a] - v0[:, a] for a in range(3))
    e2 = tuple(v2[:, a] - v0[:, a] for a in range(3))
    c = _cross(e1, e2)
    il = np.float32(1.0) / np.sqrt(_dot(c, c))
    out[h] = np.stack([c[0] * il, c[1] * il, c[2] * il], axis=1)
    return out
