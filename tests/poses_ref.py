"""Numpy float32 restatement of the pose queries on a sampled field (vx_field_poses, csrc/vx_poses.h), for the tests.

S is the signed field of a grid, float32[Z, Y, X], as field_ref takes it.  Every intermediate is float32, in the order the contract
writes it.  The reduction is restated on the floats themselves -- the smallest g, then the lowest index that has it -- not on the
integer keys the kernels use.
"""
import numpy as np

import field_ref as fr

F = np.float32
NO_POINT = 0xFFFFFFFF


def transform_points(transforms, points):
    """q[n, i, a] = ((m[4a] p0 + m[4a+1] p1) + m[4a+2] p2) + m[4a+3]  -> f32[N, P, 3]"""
    m = np.asarray(transforms, dtype=F).reshape(-1, 3, 4)
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        t0 = (m[:, None, :, 0] * p[None, :, 0, None]).astype(F)
        t1 = (m[:, None, :, 1] * p[None, :, 1, None]).astype(F)
        t2 = (m[:, None, :, 2] * p[None, :, 2, None]).astype(F)
        q = (((t0 + t1).astype(F) + t2).astype(F) + m[:, None, :, 3]).astype(F)
    return q


def gaps(S, org, vs, points, transforms, radii=None):
    """g[n, i] = (value(q) - radius[i]) + 0.0f  -> f32[N, P], and q f32[N, P, 3]"""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    q = transform_points(transforms, p)
    N, P = q.shape[:2]
    r = np.zeros(P, dtype=F) if radii is None else np.asarray(radii, dtype=F).reshape(P)
    v = fr.value(S, org, vs, q.reshape(-1, 3)).reshape(N, P)
    with np.errstate(over="ignore", invalid="ignore"):
        g = ((v - r[None, :]).astype(F) + F(0)).astype(F)
    return g, q


def poses(S, org, vs, points, transforms, radii=None, margin=0.0):
    """-> clearance f32[N], point u32[N], count u32[N], position f32[N, 3], gradient f32[N, 3]"""
    g, q = gaps(S, org, vs, points, transforms, radii)
    N, P = g.shape
    skip = np.isnan(g)
    some = ~skip.all(axis=1) if P else np.zeros(N, dtype=bool)
    clearance = np.full(N, np.inf, dtype=F)
    point = np.full(N, NO_POINT, dtype=np.uint32)
    count = np.zeros(N, dtype=np.uint32)
    position = np.zeros((N, 3), dtype=F)
    gradient = np.zeros((N, 3), dtype=F)
    if P:
        with np.errstate(invalid="ignore"):
            count[:] = (~skip & (g <= F(margin))).sum(axis=1)
        gi = np.where(skip, F(np.inf), g)
        lo = gi.min(axis=1)
        # the lowest index among the points not skipped whose g equals the smallest (np.argmax: the first True)
        first = np.argmax(~skip & (gi == lo[:, None]), axis=1)
        clearance[some] = lo[some]
        point[some] = first[some].astype(np.uint32)
        position[some] = q[np.nonzero(some)[0], first[some]]
        gradient[some] = fr.sample(S, org, vs, position[some])[1]
    return clearance, point, count, position, gradient
