"""Reference for the multi-hit ray queries on triangles (vx_bvh_trace_multi*, vx_tlas_trace_multi*): the numpy float32 brute force of
tests/mesh_ref.py (the pinned Moeller-Trumbore over ALL triangles) and tests/instance_ref.py (the pinned object-space rays), keeping every
accepted (t, u, v) instead of the closest one, then the (t, instance, prim) order, the cursor, truncation to K and the padding of
include/voxhip.h.  A helper for the tests, not a test itself.

all_hits / all_hits_tlas compute the accepted hits of a ray batch once; select() applies K and the cursor to them."""
import numpy as np

import instance_ref
import mesh_ref

F = np.float32
NONE = np.uint32(0xFFFFFFFF)


class Hits:
    """every accepted hit of a batch of n rays, sorted by (ray, t, instance, prim)"""

    def __init__(self, n, ray, t, inst, prim, u, v):
        o = np.lexsort((prim, inst, t, ray))
        self.n = n
        self.ray, self.t, self.inst, self.prim, self.u, self.v = (np.ascontiguousarray(a[o]) for a in (ray, t, inst, prim, u, v))
        assert self.t.dtype == F and self.u.dtype == F and self.v.dtype == F


def _accepted(verts, tris, rays, tmin, tmax, tmax_per_ray):
    """(ray, t, prim, u, v) of every accepted (ray, triangle) pair, chunked as mesh_ref.closest chunks"""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n = rays.shape[0]
    nt = int(np.asarray(tris).reshape(-1, 3).shape[0])
    parts = []
    if nt and n:
        tri = mesh_ref._tris(verts, tris)
        for i, j in mesh_ref._chunks(n, nt):
            lo, hi = mesh_ref._bounds(rays, tmin, tmax, tmax_per_ray, i, j)
            acc, t, u, v = mesh_ref._mt(tri, rays[i:j], lo, hi)
            rr, kk = np.nonzero(acc)
            parts.append((rr + i, t[rr, kk], kk, u[rr, kk], v[rr, kk]))
    if not parts:
        z = np.zeros(0, np.int64)
        return z, np.zeros(0, F), z, np.zeros(0, F), np.zeros(0, F)
    return tuple(np.concatenate([p[c] for p in parts]) for c in range(5))


def all_hits(verts, tris, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    """one mesh: the instance part of every key is 0"""
    n = np.asarray(rays).reshape(-1, 6).shape[0]
    ray, t, prim, u, v = _accepted(verts, tris, rays, tmin, tmax, tmax_per_ray)
    return Hits(n, ray, t, np.zeros(len(ray), np.int64), prim, u, v)


def all_hits_tlas(meshes, inst, rays, tmin=0.001, tmax=10000.0, tmax_per_ray=None):
    """meshes[b] = (verts, tris) of BLAS b; every active (instance, triangle) pair on the instance's object-space ray"""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    w, _ = instance_ref.inverse(inst["transform"])
    act = instance_ref.active(inst, [len(np.asarray(tr).reshape(-1, 3)) for _, tr in meshes])
    parts = []
    for i in np.nonzero(act)[0]:
        vv, tr = meshes[int(inst["blas"][i])]
        ray, t, prim, u, v = _accepted(vv, tr, instance_ref.object_rays(w[i], rays), tmin, tmax, tmax_per_ray)
        parts.append((ray, t, np.full(len(ray), i, np.int64), prim, u, v))
    if not parts:
        z = np.zeros(0, np.int64)
        return Hits(len(rays), z, np.zeros(0, F), z, z, np.zeros(0, F), np.zeros(0, F))
    return Hits(len(rays), *(np.concatenate([p[c] for p in parts]) for c in range(6)))


def select(h, k, after=None):
    """The contract on the hits of a batch -> dict: t [n, k] float32, instance / prim [n, k] uint32, bary [n, k, 2] float32, count [n] uint32.
    after = (after_t, after_prim) or (after_t, after_instance, after_prim), one entry per ray each."""
    n = h.n
    keep = np.ones(len(h.ray), bool)
    if after is not None:
        at = np.asarray(after[0], F)[h.ray]
        ap = np.asarray(after[-1], np.uint32).astype(np.int64)[h.ray]
        ai = np.asarray(after[1], np.uint32).astype(np.int64)[h.ray] if len(after) == 3 else np.zeros(len(h.ray), np.int64)
        keep = (h.t > at) | ((h.t == at) & ((h.inst > ai) | ((h.inst == ai) & (h.prim > ap))))
    ray = h.ray[keep]
    count = np.bincount(ray, minlength=n).astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(count.astype(np.int64))])[:-1]
    rank = np.arange(len(ray)) - start[ray]
    top = rank < k
    r, j = ray[top], rank[top]
    out = {"t": np.full((n, k), F(-1), F), "instance": np.full((n, k), NONE, np.uint32), "prim": np.full((n, k), NONE, np.uint32),
           "bary": np.zeros((n, k, 2), F), "count": count}
    out["t"][r, j] = h.t[keep][top]
    out["instance"][r, j] = h.inst[keep][top].astype(np.uint32)
    out["prim"][r, j] = h.prim[keep][top].astype(np.uint32)
    out["bary"][r, j, 0] = h.u[keep][top]
    out["bary"][r, j, 1] = h.v[keep][top]
    return out


def cursor_of(page, prev=None, tlas=False):
    """the cursor behind a page: its last listed hit per ray; rays whose page is empty keep `prev` (or (-1, ...): no cursor)"""
    t = page["t"]
    n, k = t.shape
    m = (t > 0).sum(axis=1)
    have = m > 0
    last = np.maximum(m - 1, 0)
    rows = np.arange(n)
    fields = ("t", "instance", "prim") if tlas else ("t", "prim")
    if prev is None:
        prev = tuple(np.full(n, F(-1), F) if f == "t" else np.zeros(n, np.uint32) for f in fields)
    return tuple(np.where(have, page[f][rows, last], p).astype(p.dtype) for f, p in zip(fields, prev))
