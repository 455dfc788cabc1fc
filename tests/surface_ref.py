"""The boundary mesh of a voxel mask (vx_grid_surface*) restated in numpy, vectorised for 512^3 masks.

cells: bool [Z, Y, X] (cell (x, y, z) at cells[z, y, x], linear index x + X*(y + Y*z)).  A face of an occupied cell in direction d (0..5 =
-X, +X, -Y, +Y, -Z, +Z) is exposed when the neighbour is outside the grid or empty.  Lattice points (i, j, k), index i + (X+1)*(j + (Y+1)*k);
the used ones (touched by a face) in ascending index are the vertices; faces in ascending cell, then d, each two triangles (c0, c1, c2),
(c0, c2, c3) over the corners of FACE_CORNERS.  Positions per axis: org + ((float)i + 0.5f) * vs - half in float32."""
import numpy as np

F = np.float32
# corners of the face in direction d as (dx, dy, dz), counter-clockwise seen from the empty side
FACE_CORNERS = np.array([
    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],   # -X
    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],   # +X
    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],   # -Y
    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],   # +Y
    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],   # -Z
    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],   # +Z
], dtype=np.int64)
DIRS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], dtype=np.int64)


def face_codes(cells):
    """uint8 [Z, Y, X]: bit d set when the cell has an exposed face in direction d."""
    c = np.ascontiguousarray(cells, dtype=bool)
    code = np.zeros(c.shape, np.uint8)
    for d, (dx, dy, dz) in enumerate(DIRS):
        axis = 2 if dx else (1 if dy else 0)
        step = int(dx + dy + dz)
        nb = np.zeros_like(c)
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        if step > 0:   # neighbour at +1: nb[i] = c[i + 1]
            dst[axis], src[axis] = slice(0, -1), slice(1, None)
        else:
            dst[axis], src[axis] = slice(1, None), slice(0, -1)
        nb[tuple(dst)] = c[tuple(src)]
        code |= ((c & ~nb).astype(np.uint8) << d)
    return code


def faces(cells):
    """(cell index (F,) int64, d (F,) int64) of every exposed face in emission order."""
    code = face_codes(cells).reshape(-1)
    idx = np.flatnonzero(code)
    bits = (code[idx][:, None] >> np.arange(6, dtype=np.uint8)) & 1
    k, d = np.nonzero(bits)  # row-major: ascending cell, then d
    return idx[k].astype(np.int64), d.astype(np.int64)


def lattice_index(ijk, dim):
    X, Y, _ = dim
    return ijk[..., 0] + (X + 1) * (ijk[..., 1] + (Y + 1) * ijk[..., 2])


def lattice_ijk(p, dim):
    X, Y, _ = dim
    p = np.asarray(p, np.int64)
    return np.stack([p % (X + 1), (p // (X + 1)) % (Y + 1), p // ((X + 1) * (Y + 1))], axis=-1)


def surface_lattice(cells):
    """-> (used lattice indices (V,) int64 ascending, tris (T, 3) int32, face cell (F,), face d (F,))."""
    Z, Y, X = cells.shape
    dim = (X, Y, Z)
    cell, d = faces(cells)
    xyz = np.stack([cell % X, (cell // X) % Y, cell // (X * Y)], axis=-1)
    corners = xyz[:, None, :] + FACE_CORNERS[d]            # (F, 4, 3)
    lat = lattice_index(corners, dim)                        # (F, 4)
    used = np.unique(lat)
    q = np.searchsorted(used, lat).astype(np.int32)
    tris = np.empty((2 * len(cell), 3), np.int32)
    tris[0::2] = q[:, [0, 1, 2]]
    tris[1::2] = q[:, [0, 2, 3]]
    return used, tris, cell, d


def positions(ijk, org, vs):
    """org + ((float)i + 0.5f) * vs - half per axis, float32, no contraction."""
    vs = F(vs)
    half = vs * F(0.5)
    out = np.empty(ijk.shape, np.float32)
    for a in range(3):
        out[:, a] = (F(org[a]) + ((ijk[:, a].astype(np.float32) + F(0.5)) * vs)) - half
    return out


def surface(cells, org, vs, cell_ids=None):
    """-> (verts (V, 3) f32, tris (T, 3) int32[, mats (T,) int32]); cell_ids: one id per occupied cell in ascending cell order."""
    Z, Y, X = cells.shape
    used, tris, cell, _ = surface_lattice(cells)
    verts = positions(lattice_ijk(used, (X, Y, Z)), org, vs)
    if cell_ids is None:
        return verts, tris
    occ = np.flatnonzero(np.ascontiguousarray(cells).reshape(-1))
    rank = np.searchsorted(occ, cell)
    ids = np.asarray(cell_ids)[rank].astype(np.int32)
    return verts, tris, np.repeat(ids, 2)


def mixed_corners(cells):
    """The 2x2x2 rule: lattice points whose eight surrounding cells (outside = empty) are neither all empty nor all occupied, ascending."""
    Z, Y, X = cells.shape
    p = np.zeros((Z + 2, Y + 2, X + 2), bool)
    p[1:-1, 1:-1, 1:-1] = cells
    cnt = np.zeros((Z + 1, Y + 1, X + 1), np.int8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cnt += p[dz:dz + Z + 1, dy:dy + Y + 1, dx:dx + X + 1]
    return np.flatnonzero(((cnt > 0) & (cnt < 8)).reshape(-1))


def brute(cells, org, vs):
    """The contract as a per-cell loop (small masks only)."""
    Z, Y, X = cells.shape
    fl = []
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                if not cells[z, y, x]:
                    continue
                for d in range(6):
                    nx, ny, nz = x + DIRS[d][0], y + DIRS[d][1], z + DIRS[d][2]
                    inside = 0 <= nx < X and 0 <= ny < Y and 0 <= nz < Z
                    if inside and cells[nz, ny, nx]:
                        continue
                    fl.append([(x + c[0]) + (X + 1) * ((y + c[1]) + (Y + 1) * (z + c[2])) for c in FACE_CORNERS[d]])
    used = sorted({p for f in fl for p in f})
    rank = {p: i for i, p in enumerate(used)}
    tris = []
    for f in fl:
        a, b, c, e = (rank[p] for p in f)
        tris += [(a, b, c), (a, c, e)]
    ijk = lattice_ijk(np.array(used, np.int64), (X, Y, Z)) if used else np.zeros((0, 3), np.int64)
    return positions(ijk, org, vs), np.array(tris, np.int32).reshape(-1, 3)


def pack(cells):
    """bool[Z, Y, X] -> uint32 words, ceil(N / 32) of them (the library's bitmask)."""
    flat = np.ascontiguousarray(cells, dtype=bool).reshape(-1)
    nw = (flat.size + 31) // 32
    b = np.packbits(flat, bitorder="little")
    out = np.zeros(nw * 4, dtype=np.uint8)
    out[:b.size] = b
    return out.view(np.uint32)


def unpack(words, dim):
    X, Y, Z = dim
    n = X * Y * Z
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[:n]
    return bits.astype(bool).reshape(Z, Y, X)
