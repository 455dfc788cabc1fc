"""Numpy restatement of solid voxelization (VX_VOXELIZE_SOLID, vx_grid_fill_interior), for the tests.

S = the surface bitmask; an empty cell is exterior when 6-connected empty cells join it to an empty cell of the grid's boundary; H = the
empty cells that are not exterior; the solid grid is S | H (scipy.ndimage.binary_fill_holes(S), without needing scipy).  The exterior is
grown from the boundary by whole runs of empty cells along x, y and z in turn (a run that holds an exterior cell is exterior) until nothing
changes.  The Vec list and the material ids of a solid build follow from the oracle's surface outputs: the build behaves as if
setVoxel(x, y, z, MaterialObj{}) ran on every cell of H in ascending voxel index after the triangle loop.
"""
import numpy as np


def unpack(words, dim):
    """uint32 bitmask (LSB first, i = x + X*(y + Y*z)) -> bool[Z, Y, X]."""
    X, Y, Z = (int(d) for d in dim)
    n = X * Y * Z
    bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:n]
    return bits.astype(bool).reshape(Z, Y, X)


def pack(cells):
    """bool[Z, Y, X] -> uint32 words, ceil(N / 32) of them."""
    flat = np.ascontiguousarray(cells, dtype=bool).reshape(-1)
    nw = (flat.size + 31) // 32
    b = np.packbits(flat, bitorder="little")
    out = np.zeros(nw * 4, dtype=np.uint8)
    out[:b.size] = b
    return out.view(np.uint32)


def _grow_along(ext, empty, axis):
    """ext |= every run of empty cells along `axis` that holds an exterior cell."""
    e = np.moveaxis(ext, axis, -1)
    p = np.moveaxis(empty, axis, -1)
    L = p.shape[-1]
    lines = p.size // L if L else 0
    run = np.cumsum(~p, axis=-1) + (np.arange(lines).reshape(p.shape[:-1]) * (L + 1))[..., None]
    seen = np.zeros(lines * (L + 1) + 1, dtype=bool)
    seen[run[e]] = True
    out = p & seen[run]
    return np.moveaxis(out, -1, axis)


def exterior(cells):
    """bool[Z, Y, X] occupancy -> bool[Z, Y, X] exterior (the empty cells joined to the boundary)."""
    empty = ~np.asarray(cells, dtype=bool)
    ext = np.zeros_like(empty)
    if empty.size == 0:
        return ext
    ext[0, :, :] = ext[-1, :, :] = True
    ext[:, 0, :] = ext[:, -1, :] = True
    ext[:, :, 0] = ext[:, :, -1] = True
    ext &= empty
    while True:
        before = int(ext.sum())
        for axis in (2, 1, 0):
            ext = _grow_along(ext, empty, axis)
        if int(ext.sum()) == before:
            return ext


def interior_cells(cells):
    cells = np.asarray(cells, dtype=bool)
    return ~cells & ~exterior(cells)


def fill(words, dim):
    """-> (solid words S | H, H words, |H|) for a bitmask of dims (X, Y, Z)."""
    s = unpack(words, dim)
    h = interior_cells(s)
    return pack(s | h), pack(h), int(h.sum())


def solid_vec(surface_vec, h_words, gi, vs):
    """The Vec list of a solid build: the triangles' records (oracle.build_vec), then one record per interior cell in ascending order."""
    import oracle
    return np.concatenate([surface_vec, oracle.bool_aabbs(h_words, gi, vs)])


def default_index(order, n_interior):
    """(index of MaterialObj{} in getMatrials(), the value order after the second loop).  Value 0 is MaterialObj{}: appended when the
    interior is not empty and no triangle used it."""
    order = [int(v) for v in order]
    if n_interior and 0 not in order:
        order.append(0)
    return (order.index(0) if 0 in order else -1), order


def solid_material_ids_bool(surface_ids, s_words, h_words, dim, order):
    """Bool / AABBstruct ids over S | H in ascending voxel order: surface voxels keep theirs, interior ones get MaterialObj{}'s."""
    s = unpack(s_words, dim).reshape(-1)
    h = unpack(h_words, dim).reshape(-1)
    nh = int(h.sum())
    d, order = default_index(order, nh)
    ids = np.full(int((s | h).sum()), -1, dtype=np.int16)
    occ = np.flatnonzero(s | h)
    is_surface = s[occ]
    ids[is_surface] = surface_ids
    ids[~is_surface] = d
    return ids, order


def solid_material_ids_vec(surface_ids, n_interior, order):
    d, order = default_index(order, n_interior)
    return np.concatenate([np.asarray(surface_ids, dtype=np.int16), np.full(n_interior, d, dtype=np.int16)]), order
