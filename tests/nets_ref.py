"""Surface nets of a voxel mask (vx_grid_surface_smooth*) restated in numpy, on top of surface_ref: the vertices, their order and the
triangles are surface_ref's; only the positions differ, and normals are added.

cells: bool [Z, Y, X].  Vertex v is lattice point p = (i, j, k); its block is the eight cells (i-1+a, j-1+b, k-1+e), configuration bit
a | b << 1 | e << 2 (cells outside the grid are empty).  An edge of the block crosses when exactly one of its two cells is occupied; n = the
crossing edges, T_A = the sum over crossing edges not along A of (2 bit_A - 1), u0_A = (float)T_A / (float)(2 n).  q = p +- e_A is a
neighbour when the four block cells on that side are mixed.  A step with weight w: s = sum over the neighbours in the order -X, +X, -Y,
+Y, -Z, +Z of u_q (plus -+1 on the direction's axis), mean = s / (float)m, t = u + w*(mean - u), u' = min(max(t, -0.5), 0.5).  One
iteration = a step with lam, then one with mu when mu != 0.  Position per axis: org + (((float)i + 0.5f) + u)*vs - half.  Normals: the
sum, over the block's mixed internal faces (axis x, y, z; the other two bits 00, 10, 01, 11), of cross(P(c2) - P(c0), P(c3) - P(c1)) of the
occupied cell's face, every product and difference rounded, divided by its length (0 when the length is 0 or not finite)."""
import numpy as np

import surface_ref as sr

F = np.float32
# the block's twelve edges as (axis, bit index of the cell with axis bit 0); the other cell is that | 1 << axis
EDGES = [(A, c) for A in range(3) for c in range(8) if not (c >> A) & 1]
# the twelve internal faces in the contract's order: axis A, then the other two bits with the first of the other axes fastest
FACES = []
for _A in range(3):
    _o = [a for a in range(3) if a != _A]
    for _hi in (0, 1):
        for _lo in (0, 1):
            FACES.append((_A, (_lo << _o[0]) | (_hi << _o[1])))


def check_params(iterations, lam, mu):
    return (0 <= iterations <= 1024 and np.isfinite(lam) and 0.0 <= lam <= 1.0 and np.isfinite(mu) and -1.0 <= mu <= 0.0)


def configs(cells):
    """uint8 [Z+1, Y+1, X+1]: the block configuration of every lattice point."""
    Z, Y, X = cells.shape
    p = np.zeros((Z + 2, Y + 2, X + 2), bool)
    p[1:-1, 1:-1, 1:-1] = cells
    cfg = np.zeros((Z + 1, Y + 1, X + 1), np.uint8)
    for c in range(8):
        a, b, e = c & 1, (c >> 1) & 1, c >> 2
        cfg |= p[e:e + Z + 1, b:b + Y + 1, a:a + X + 1].astype(np.uint8) << c
    return cfg


def _tables():
    n = np.zeros(256, np.int32)
    T = np.zeros((256, 3), np.int32)
    nb = np.zeros((256, 6), bool)
    for cfg in range(256):
        bit = lambda c: (cfg >> c) & 1
        for A, c in EDGES:
            if bit(c) == bit(c | (1 << A)):
                continue
            n[cfg] += 1
            for B in range(3):
                if B != A:
                    T[cfg, B] += 2 * ((c >> B) & 1) - 1
        for d in range(6):
            A, side = d // 2, d % 2
            s = sum(bit(c) for c in range(8) if ((c >> A) & 1) == side)
            nb[cfg, d] = 0 < s < 4
    return n, T, nb


N_TAB, T_TAB, NB_TAB = _tables()


def topology(cells):
    """-> used (V,) lattice indices, ijk (V, 3), cfg (V,) uint8, nbr (V, 6) int64 vertex index or -1"""
    Z, Y, X = cells.shape
    cfg_all = configs(cells).reshape(-1)
    used = np.flatnonzero((cfg_all != 0) & (cfg_all != 255))
    cfg = cfg_all[used]
    ijk = sr.lattice_ijk(used, (X, Y, Z)) if len(used) else np.zeros((0, 3), np.int64)
    step = np.array([1, X + 1, (X + 1) * (Y + 1)], np.int64)
    nbr = np.full((len(used), 6), -1, np.int64)
    for d in range(6):
        has = NB_TAB[cfg, d]
        q = used[has] + (2 * (d % 2) - 1) * step[d // 2]
        r = np.searchsorted(used, q)
        assert (used[r] == q).all()
        nbr[has, d] = r
    return used, ijk, cfg, nbr


def initial(cfg):
    """u0 (V, 3) float32"""
    n = N_TAB[cfg]
    return (T_TAB[cfg].astype(np.float32) / (2 * n).astype(np.float32)[:, None]).astype(np.float32)


def step(u, nbr, w):
    w = F(w)
    s = np.zeros_like(u)
    m = (nbr >= 0).sum(axis=1)
    for d in range(6):
        has = nbr[:, d] >= 0
        r = u[nbr[has, d]].copy()
        r[:, d // 2] = F(2 * (d % 2) - 1) + r[:, d // 2]
        s[has] = s[has] + r
    mean = s / m.astype(np.float32)[:, None]
    t = u + w * (mean - u)
    return np.minimum(np.maximum(t, F(-0.5)), F(0.5)).astype(np.float32)


def relax(u, nbr, iterations, lam, mu):
    for _ in range(iterations):
        u = step(u, nbr, lam)
        if F(mu) != 0:
            u = step(u, nbr, mu)
    return u


def positions(ijk, u, org, vs):
    vs = F(vs)
    half = vs * F(0.5)
    out = np.empty(u.shape, np.float32)
    for a in range(3):
        out[:, a] = (F(org[a]) + (((ijk[:, a].astype(np.float32) + F(0.5)) + u[:, a]) * vs)) - half
    return out


def _face_corners(ijk, cfg, f, dim):
    """counted (V,) bool and the four corners' lattice indices (V, 4) of internal face f of every block (garbage where not counted)"""
    A, c = FACES[f]
    lo, hi = (cfg >> c) & 1, (cfg >> (c | (1 << A))) & 1
    counted = lo != hi
    cell_bits = np.where(lo == 1, c, c | (1 << A))         # the occupied cell of the pair
    d = 2 * A + (lo == 1)                                   # its +A face when it is the low cell
    cb = np.stack([cell_bits & 1, (cell_bits >> 1) & 1, cell_bits >> 2], axis=-1).astype(np.int64)
    cell = ijk - 1 + cb                                      # (V, 3)
    corners = cell[:, None, :] + sr.FACE_CORNERS[d]         # (V, 4, 3)
    return counted, sr.lattice_index(corners, dim)


def normals(used, ijk, cfg, P, dim):
    V = len(used)
    N = np.zeros((V, 3), np.float32)
    for f in range(12):
        counted, lat = _face_corners(ijk, cfg, f, dim)
        if not counted.any():
            continue
        q = np.searchsorted(used, lat[counted])
        assert (used[q] == lat[counted]).all()
        a = P[q[:, 2]] - P[q[:, 0]]
        b = P[q[:, 3]] - P[q[:, 1]]
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=-1)
        N[counted] = N[counted] + c.astype(np.float32)
    with np.errstate(all="ignore"):
        l = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = (l > 0) & np.isfinite(l)
        out = np.zeros_like(N)
        out[ok] = N[ok] / l[ok][:, None]
    return out


def offsets(cells, iterations=8, lam=0.5, mu=-0.53):
    """-> used, ijk, cfg, nbr, u0, u"""
    assert check_params(iterations, lam, mu)
    used, ijk, cfg, nbr = topology(cells)
    u0 = initial(cfg)
    return used, ijk, cfg, nbr, u0, relax(u0, nbr, iterations, lam, mu)


def surface_smooth(cells, org, vs, iterations=8, lam=0.5, mu=-0.53, cell_ids=None, with_normals=False):
    """-> (verts (V, 3) f32, tris (T, 3) int32[, mats (T,) int32][, normals (V, 3) f32])"""
    Z, Y, X = cells.shape
    base = sr.surface(cells, org, vs, cell_ids=cell_ids)
    used, ijk, cfg, _, _, u = offsets(cells, iterations, lam, mu)
    P = positions(ijk, u, org, vs)
    out = (P,) + tuple(base[1:])
    if with_normals:
        out += (normals(used, ijk, cfg, P, (X, Y, Z)),)
    return out


# ---- the contract as a per-vertex loop (small masks only) ------------------------------------------------------------------------
def brute(cells, org, vs, iterations, lam, mu):
    """-> verts, normals, u0, u, n (V,), m (V,), used"""
    Z, Y, X = cells.shape
    lam, mu, vs = F(lam), F(mu), F(vs)
    half = vs * F(0.5)

    def occ(x, y, z):
        return bool(0 <= x < X and 0 <= y < Y and 0 <= z < Z and cells[z, y, x])

    verts = {}
    order = []
    for k in range(Z + 1):
        for j in range(Y + 1):
            for i in range(X + 1):
                blk = [occ(i - 1 + (c & 1), j - 1 + ((c >> 1) & 1), k - 1 + (c >> 2)) for c in range(8)]
                if any(blk) and not all(blk):
                    verts[(i, j, k)] = blk
                    order.append((i, j, k))
    index = {p: v for v, p in enumerate(order)}
    V = len(order)
    u0 = np.zeros((V, 3), np.float32)
    ns, nbrs = [], []
    for v, p in enumerate(order):
        blk = verts[p]
        n, T = 0, [0, 0, 0]
        for A in range(3):
            for c in range(8):
                if (c >> A) & 1 or blk[c] == blk[c | (1 << A)]:
                    continue
                n += 1
                for B in range(3):
                    if B != A:
                        T[B] += 2 * ((c >> B) & 1) - 1
        ns.append(n)
        for A in range(3):
            u0[v, A] = F(T[A]) / F(2 * n)
        nb = []
        for d in range(6):
            A, side = d // 2, d % 2
            four = [blk[c] for c in range(8) if ((c >> A) & 1) == side]
            if any(four) and not all(four):
                q = list(p)
                q[A] += 2 * side - 1
                nb.append((d, index[tuple(q)]))
        nbrs.append(nb)

    def one(u, w):
        out = np.empty_like(u)
        for v in range(V):
            s = [F(0), F(0), F(0)]
            for d, q in nbrs[v]:
                for A in range(3):
                    r = u[q, A]
                    if A == d // 2:
                        r = F(2 * (d % 2) - 1) + r
                    s[A] = s[A] + r
            for A in range(3):
                mean = s[A] / F(len(nbrs[v]))
                t = u[v, A] + w * (mean - u[v, A])
                out[v, A] = min(max(t, F(-0.5)), F(0.5))
        return out

    u = u0.copy()
    for _ in range(iterations):
        u = one(u, lam)
        if mu != 0:
            u = one(u, mu)
    P = np.empty((V, 3), np.float32)
    for v, p in enumerate(order):
        for A in range(3):
            P[v, A] = (F(org[A]) + ((F(p[A]) + F(0.5)) + u[v, A]) * vs) - half
    Nn = np.zeros((V, 3), np.float32)
    with np.errstate(all="ignore"):
        for v, p in enumerate(order):
            blk = verts[p]
            N = [F(0), F(0), F(0)]
            for A in range(3):
                o = [a for a in range(3) if a != A]
                for hi2 in (0, 1):
                    for lo2 in (0, 1):
                        c = (lo2 << o[0]) | (hi2 << o[1])
                        c1 = c | (1 << A)
                        if blk[c] == blk[c1]:
                            continue
                        cc, d = (c, 2 * A + 1) if blk[c] else (c1, 2 * A)
                        cell = [p[0] - 1 + (cc & 1), p[1] - 1 + ((cc >> 1) & 1), p[2] - 1 + (cc >> 2)]
                        q = [P[index[tuple(int(cell[a] + sr.FACE_CORNERS[d][e][a]) for a in range(3))]] for e in range(4)]
                        a_, b_ = q[2] - q[0], q[3] - q[1]
                        N[0] = N[0] + (a_[1] * b_[2] - a_[2] * b_[1])
                        N[1] = N[1] + (a_[2] * b_[0] - a_[0] * b_[2])
                        N[2] = N[2] + (a_[0] * b_[1] - a_[1] * b_[0])
            l = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
            if l > 0 and np.isfinite(l):
                Nn[v] = [N[0] / l, N[1] / l, N[2] / l]
    used = np.array([i + (X + 1) * (j + (Y + 1) * k) for i, j, k in order], np.int64)
    return P, Nn, u0, u, np.array(ns), np.array([len(b) for b in nbrs]), used
