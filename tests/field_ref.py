"""Numpy float32 restatement of the sampled signed field and the sphere cast (vx_field, csrc/vx_field.h), for the tests.

S is the signed field of a grid, float32[Z, Y, X] (distance_ref.sdf_from, or the GPU's own sdf()).  Every intermediate is float32, in the
order the contract writes it; fmin / fmax are np.fmin / np.fmax (a NaN operand is ignored, as fminf / fmaxf do).
"""
import numpy as np

import distance_ref

F = np.float32
FINITE, EMPTY, FULL = 0, 1, 2
MISS, HIT, STEP_LIMIT = 0, 1, 2
NAN_BITS = 0x7FC00000


def field_of_mask(m, vs):
    """bool[Z, Y, X] -> the signed field float32[Z, Y, X]."""
    m = np.asarray(m, dtype=bool)
    return distance_ref.sdf_from(m, distance_ref.edt_sq_c(m), distance_ref.edt_sq_c(~m), vs)


def state_of(S):
    if np.all(np.isposinf(S)):
        return EMPTY
    if np.all(np.isneginf(S)):
        return FULL
    return FINITE


def _axis(p, org, vs, dim):
    with np.errstate(over="ignore", invalid="ignore"):
        top = F(dim - 1)
        u_raw = ((p - F(org)) / F(vs)).astype(F) - F(0.5)
        out = (u_raw < F(0)) | (u_raw > top) | (dim == 1)
        u = np.fmin(np.fmax(u_raw, F(0)), top).astype(F)
        i0 = np.minimum(np.nan_to_num(u, nan=0.0).astype(np.uint32).astype(np.int64), max(dim - 2, 0))
        i1 = np.minimum(i0 + 1, dim - 1)
        f = (u - i0.astype(F)).astype(F)
    return i0, i1, f, out


def _lerp(a, b, f):
    return (a + (f * (b - a).astype(F)).astype(F)).astype(F)


def sample(S, org, vs, points):
    """-> value f32[n], gradient f32[n, 3], occupied u8[n]"""
    S = np.asarray(S, dtype=F)
    Z, Y, X = S.shape
    dim = (X, Y, Z)
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    vs = F(vs)
    st = state_of(S)
    bad = ~np.isfinite(p).all(axis=1)
    q = np.where(bad[:, None], F(0), p).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        cellf = [((q[:, a] - F(org[a])) / vs).astype(F) for a in range(3)]
        inbox = np.ones(n, dtype=bool)
        for a in range(3):
            inbox &= (cellf[a] >= F(0)) & (cellf[a] < F(dim[a]))
        ci = [np.where(inbox, cellf[a], F(0)).astype(np.uint32).astype(np.int64) for a in range(3)]
    grad = np.zeros((n, 3), dtype=F)
    if st != FINITE:
        value = np.full(n, np.inf if st == EMPTY else -np.inf, dtype=F)
        occ = (inbox & (st == FULL))
    else:
        ax = [_axis(q[:, a], org[a], vs, dim[a]) for a in range(3)]
        (x0, x1, fx, ox), (y0, y1, fy, oy), (z0, z1, fz, oz) = ax
        c000, c100 = S[z0, y0, x0], S[z0, y0, x1]
        c010, c110 = S[z0, y1, x0], S[z0, y1, x1]
        c001, c101 = S[z1, y0, x0], S[z1, y0, x1]
        c011, c111 = S[z1, y1, x0], S[z1, y1, x1]
        value = _lerp(_lerp(_lerp(c000, c100, fx), _lerp(c010, c110, fx), fy), _lerp(_lerp(c001, c101, fx), _lerp(c011, c111, fx), fy), fz)
        gx = (_lerp(_lerp(c100 - c000, c110 - c010, fy), _lerp(c101 - c001, c111 - c011, fy), fz) / vs).astype(F)
        gy = (_lerp(_lerp(c010 - c000, c110 - c100, fx), _lerp(c011 - c001, c111 - c101, fx), fz) / vs).astype(F)
        gz = (_lerp(_lerp(c001 - c000, c101 - c100, fx), _lerp(c011 - c010, c111 - c110, fx), fy) / vs).astype(F)
        grad[:, 0] = np.where(ox, F(0), gx)
        grad[:, 1] = np.where(oy, F(0), gy)
        grad[:, 2] = np.where(oz, F(0), gz)
        occ = inbox & (S[ci[2], ci[1], ci[0]] < F(0))
    value = value.copy()
    value.view(np.uint32)[bad] = NAN_BITS
    grad[bad] = F(0)
    occ = np.where(bad, False, occ)
    return value, grad, occ.astype(np.uint8)


def value(S, org, vs, points):
    return sample(S, org, vs, points)[0]


def sphere_trace(S, org, vs, rays, radius=0.0, radius_per_ray=None, tmin=0.001, tmax=10000.0, tmax_per_ray=None, step_scale=0.25, hit_eps=1.0 / 64,
                 max_steps=256):
    """-> t f32[n], clearance f32[n], steps u32[n], status u8[n]"""
    S = np.asarray(S, dtype=F)
    Z, Y, X = S.shape
    dim = (X, Y, Z)
    r = np.asarray(rays, dtype=F).reshape(-1, 6)
    n = r.shape[0]
    o, d = r[:, :3], r[:, 3:]
    vs = F(vs)
    rad = np.full(n, radius, dtype=F) if radius_per_ray is None else np.asarray(radius_per_ray, dtype=F)
    t1 = np.full(n, tmax, dtype=F) if tmax_per_ray is None else np.asarray(tmax_per_ray, dtype=F).copy()
    t0 = np.full(n, tmin, dtype=F)
    eps = F(F(hit_eps) * vs)
    scale = F(step_scale)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        miss = ~np.isfinite(r).all(axis=1)
        miss |= ~(rad >= F(0)) | np.isinf(rad)
        dn = np.sqrt((((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)).astype(F)
        miss |= ~(dn > F(0)) | np.isinf(dn)
        for a in range(3):
            lo = F(org[a])
            hi = F(lo + F(F(dim[a]) * vs))
            inv = (F(1) / d[:, a]).astype(F)
            deg = np.isinf(inv)
            miss |= deg & ~((lo <= o[:, a]) & (o[:, a] <= hi))
            ta = ((lo - o[:, a]).astype(F) * inv).astype(F)
            tb = ((hi - o[:, a]).astype(F) * inv).astype(F)
            t0 = np.where(deg, t0, np.fmax(t0, np.fmin(ta, tb))).astype(F)
            t1 = np.where(deg, t1, np.fmin(t1, np.fmax(ta, tb))).astype(F)
        miss |= ~(t0 <= t1)
        t_out = np.full(n, -1, dtype=F)
        clr = np.full(n, np.inf, dtype=F)
        steps = np.zeros(n, dtype=np.uint32)
        status = np.full(n, MISS, dtype=np.uint8)
        live = np.nonzero(~miss)[0]
        status[live] = STEP_LIMIT
        t = t0.copy()
        for k in range(max_steps):
            if live.size == 0:
                break
            tl = t[live]
            p = np.stack([(o[live, a] + (tl * d[live, a]).astype(F)).astype(F) for a in range(3)], axis=1)
            f = value(S, org, vs, p)
            steps[live] = k + 1
            clr[live] = np.fmin(clr[live], f)
            g = (f - rad[live]).astype(F)
            hit = g <= eps
            t_out[live[hit]] = tl[hit]
            status[live[hit]] = HIT
            tn = (tl + ((g * scale).astype(F) / dn[live]).astype(F)).astype(F)
            gone = ~hit & (tn > t1[live])
            status[live[gone]] = MISS
            t[live] = tn
            live = live[~hit & ~gone]
    return t_out, clr, steps, status
