"""Reference for the multi-hit ray query (vx_trace_multi*): a numpy float32 restatement of hitAabb (raytrace.rint:46-56, vx_math.h hit_aabb)
over an AABB list, then the acceptance rule, the (t, prim) order, the cursor, truncation to K and the padding of include/voxhip.h.

Every product and difference is a float32 operation; minima and maxima are np.fmin / np.fmax, which skip NaN as fminf / fmaxf do, so an
axis with 0 * inf behaves as in vx_math.h."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)


def pack(cells):
    """bool [Z, Y, X] -> the grid's bitmask words (cell x + X*(y + Y*z) = bit i % 32 of word i / 32)"""
    b = np.packbits(np.ascontiguousarray(cells, bool).ravel(), bitorder="little")
    b = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)])
    return b.view(np.uint32)


def hit_times(aabbs, rays, chunk=64):
    """t = hitAabb(box, ray) for every ray and box -> float32 [R, N] (-1: no hit)"""
    r = np.ascontiguousarray(rays, F).reshape(-1, 6)
    mn = np.ascontiguousarray(aabbs["mn"], F).reshape(-1, 3)
    mx = np.ascontiguousarray(aabbs["mx"], F).reshape(-1, 3)
    out = np.empty((len(r), len(mn)), F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(0, len(r), chunk):
            o = r[s:s + chunk, None, :3]
            inv = (F(1) / r[s:s + chunk, 3:])[:, None, :]          # invDir = 1.0 / dir
            tbot = inv * (mn[None] - o)
            ttop = inv * (mx[None] - o)
            lo, hi = np.fmin(ttop, tbot), np.fmax(ttop, tbot)
            t0 = np.fmax(lo[..., 0], np.fmax(lo[..., 1], lo[..., 2]))
            t1 = np.fmin(hi[..., 0], np.fmin(hi[..., 1], hi[..., 2]))
            out[s:s + chunk] = np.where(t1 > np.fmax(t0, F(0)), t0, F(-1))
    assert out.dtype == F
    return out


def select(times, k, tmin=0.001, tmax=10000.0, tmax_per_ray=None, after=None):
    """The contract on a matrix of hit_times: -> t [R, k] float32, prim [R, k] uint32, count [R] uint32"""
    R, N = times.shape
    t_out = np.full((R, k), F(-1), F)
    p_out = np.full((R, k), NONE, np.uint32)
    count = np.zeros(R, np.uint32)
    prim = np.arange(N, dtype=np.uint32)
    tmin = F(tmin)
    for r in range(R):
        t = times[r]
        hi = F(tmax) if tmax_per_ray is None else F(tmax_per_ray[r])
        with np.errstate(invalid="ignore"):
            acc = (t > F(0)) & (t >= tmin) & (t <= hi)
            if after is not None:
                at, ap = F(after[0][r]), np.uint32(after[1][r])
                acc &= (t > at) | ((t == at) & (prim > ap))
        idx = np.flatnonzero(acc)
        idx = idx[np.lexsort((prim[idx], t[idx]))]   # by t, ties by prim
        count[r] = len(idx)
        m = min(k, len(idx))
        t_out[r, :m] = t[idx[:m]]
        p_out[r, :m] = prim[idx[:m]]
    return t_out, p_out, count


def multi(aabbs, rays, k, **kw):
    return select(hit_times(aabbs, rays), k, **kw)
