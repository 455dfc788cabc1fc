"""Geometries, point sets and ray batches of the distance-field query tests (test_field_cpu.py, test_gpu_field.py)."""
import numpy as np

F = np.float32
ORG = (0.25, -1.0, 3.0)
VS_ODD, VS_DYADIC = F(0.37), F(0.5)


def prototype_mask(dims=(40, 36, 31), seed=5):
    """a ball, a one-cell plate and 0.2 % noise cells -> bool[Z, Y, X]"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    r = 0.3 * min(X, Y, Z)
    m = (x - 0.4 * X) ** 2 + (y - 0.5 * Y) ** 2 + (z - 0.55 * Z) ** 2 <= r * r
    m |= (z == Z // 5) & (x > X // 8) & (x < X - X // 8) & (y > Y // 6)
    m |= np.random.default_rng(seed).random((Z, Y, X)) < 0.002
    return m


def box(dims, org, vs):
    lo = np.array(org, dtype=F)
    hi = (lo + np.array(dims, dtype=F) * F(vs)).astype(F)
    return lo, hi


def cell_centres(dims, org, vs):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    c = [(F(org[a]) + ((i.astype(F) + F(0.5)) * F(vs)).astype(F)).astype(F) for a, i in enumerate((x, y, z))]
    return np.stack(c, axis=-1).reshape(-1, 3).astype(F)


def random_points(dims, org, vs, n, seed, grow_cells=1.0):
    lo, hi = box(dims, org, vs)
    g = F(grow_cells) * F(vs)
    return (np.random.default_rng(seed).random((n, 3)) * (hi - lo + 2 * g) + (lo - g)).astype(F)


def edge_points(dims, org, vs):
    """box corners, the bounds of the centre box with their float neighbours on both sides, points 10 boxes away, non-finite components"""
    lo, hi = box(dims, org, vs)
    mid = ((lo + hi) * F(0.5)).astype(F)
    pts = [[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)]
    for a in range(3):
        c0 = F(F(org[a]) + F(0.5) * F(vs))
        c1 = F(F(org[a]) + F(F(dims[a] - 1) + F(0.5)) * F(vs))
        for c in (c0, c1, lo[a], hi[a]):
            for v in (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))):
                p = mid.copy()
                p[a] = v
                pts.append(p)
        for s in (-10.0, 10.0):
            p = mid.copy()
            p[a] = F(mid[a] + F(s) * (hi[a] - lo[a]))
            pts.append(p)
        for v in (np.nan, np.inf, -np.inf):
            p = mid.copy()
            p[a] = v
            pts.append(p)
    pts.append([np.nan, np.inf, -np.inf])
    pts.append((mid + (hi - lo) * F(10)).astype(F))
    return np.array(pts, dtype=F)


def random_rays(dims, org, vs, n, seed, grow=1.0):
    """rays between two random points of the box grown by `grow` world units: all of them pass through the grown box"""
    lo, hi = box(dims, org, vs)
    rng = np.random.default_rng(seed)
    a = rng.random((n, 3)) * (hi - lo + 2 * grow) + (lo - grow)
    b = rng.random((n, 3)) * (hi - lo + 2 * grow) + (lo - grow)
    d = b - a
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = a - d * rng.random((n, 1)) * 2.0
    return np.concatenate([o, d], axis=1).astype(F)


def special_rays(m, org, vs):
    """rays from inside occupied cells, axis-parallel rays in and out of the slab, denormal direction components, non-finite rays"""
    Z, Y, X = m.shape
    lo, hi = box((X, Y, Z), org, vs)
    mid = ((lo + hi) * F(0.5)).astype(F)
    rays = []
    occ = np.argwhere(m)
    rng = np.random.default_rng(3)
    for z, y, x in occ[rng.permutation(len(occ))[:16]]:
        c = [F(org[a]) + (F(i) + F(0.5)) * F(vs) for a, i in enumerate((x, y, z))]
        d = rng.normal(size=3)
        rays.append(list(c) + list(d / np.linalg.norm(d)))
    for a in range(3):
        for sign in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a] = sign
            o = mid.copy()
            o[a] = lo[a] - F(1) if sign > 0 else hi[a] + F(1)
            rays.append(list(o) + d)                                # through the middle
            o2 = o.copy()
            o2[(a + 1) % 3] = hi[(a + 1) % 3] + F(0.5)              # zero component, origin outside that slab
            rays.append(list(o2) + d)
            o3 = o.copy()
            o3[(a + 1) % 3] = hi[(a + 1) % 3]                       # on the slab's face
            rays.append(list(o3) + d)
            dd = list(d)
            dd[(a + 1) % 3] = 1e-42                                 # denormal components
            dd[(a + 2) % 3] = -3e-39
            rays.append(list(o) + dd)
    rays.append(list(mid) + [0.0, 0.0, 0.0])
    rays.append(list(mid) + [1e-30, 0.0, 0.0])                      # |d|^2 underflows: dn == 0
    rays.append(list(lo - F(1)) + [3e38, 3e38, 3e38])               # dn overflows
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = list(lo - F(1)) + [1.0, 1.0, 1.0]
            r[k] = v
            rays.append(r)
    return np.array(rays, dtype=F)
