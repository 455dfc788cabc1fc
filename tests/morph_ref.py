"""Numpy restatements of the morphology (vx_grid_morph*, vx_grid_seal), for the tests.  Masks are bool[Z, Y, X].

B(r2) = {b in Z^3 : bx^2 + by^2 + bz^2 <= r2}, R = floor(sqrt(r2)).  Every operation is the operation on the infinite lattice, where every
cell outside the grid is empty, restricted to the grid.

Two forms:
  the definition   OR / AND of shifted copies over the ball's offsets, with explicit padding for close and seal and solid_ref's fill:
                   dilate, erode, open, close, seal
  the fast form    thresholds of distance_ref's fields plus the box rule (a cell nearer than R to the border loses an erosion):
                   dilate_fast, erode_fast, open_fast, close_fast, seal_fast (c=True: distance_ref's C helper, for large grids)
No scipy.
"""
import math

import numpy as np

import distance_ref
import solid_ref

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3


def radius(r2):
    return math.isqrt(int(r2))


def ball(r2):
    """the offsets (dz, dy, dx) of B(r2)"""
    R = radius(r2)
    return [(dz, dy, dx) for dz in range(-R, R + 1) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dx * dx + dy * dy + dz * dz <= r2]


def _windows(p, R, shape, r2):
    """p holds R more cells on every side than the domain `shape`: the views p[c + b], c over that domain, one per b in B(r2)"""
    Z, Y, X = shape
    for dz, dy, dx in ball(r2):
        yield p[R + dz:R + dz + Z, R + dy:R + dy + Y, R + dx:R + dx + X]


def dilate_unrestricted(m, r2):
    """the dilation on Z^3 of a mask whose outside is empty, on the domain padded by R on every side (its whole support)"""
    m = np.asarray(m, dtype=bool)
    R = radius(r2)
    shape = tuple(s + 2 * R for s in m.shape)
    p = np.pad(m, 2 * R)
    out = np.zeros(shape, dtype=bool)
    for w in _windows(p, R, shape, r2):
        out |= w
    return out


def crop(a, n):
    return a[n:a.shape[0] - n, n:a.shape[1] - n, n:a.shape[2] - n] if n else a


def dilate(m, r2):
    return crop(dilate_unrestricted(m, r2), radius(r2))


def erode(m, r2):
    """{c : every b in B has c + b in m}, cells outside m's domain empty"""
    m = np.asarray(m, dtype=bool)
    R = radius(r2)
    p = np.pad(m, R)
    out = np.ones(m.shape, dtype=bool)
    for w in _windows(p, R, m.shape, r2):
        out &= w
    return out


def open_(m, r2):
    return dilate(erode(m, r2), r2)


def close(m, r2):
    return crop(erode(dilate_unrestricted(m, r2), r2), radius(r2))


def seal(m, r2):
    m = np.asarray(m, dtype=bool)
    P = radius(r2) + 1
    d = dilate(np.pad(m, P), r2)
    f = d | solid_ref.interior_cells(d)
    return m | crop(erode(f, r2), P)


def apply(op, m, r2):
    return (dilate, erode, open_, close)[op](m, r2)


# ---- the fast form ----------------------------------------------------------------------------------------------------------------
def _edt(target, c):
    return (distance_ref.edt_sq_c if c else distance_ref.edt_sq)(target)


def box(shape, R):
    """cells at least R from every border"""
    out = np.zeros(shape, dtype=bool)
    Z, Y, X = shape
    if Z > 2 * R and Y > 2 * R and X > 2 * R:
        out[R:Z - R, R:Y - R, R:X - R] = True
    return out


def dilate_fast(m, r2, c=False):
    m = np.asarray(m, dtype=bool)
    return _edt(m, c) <= np.uint32(r2)   # (no occupied cell: the sentinel, above every r2 the library accepts)


def erode_fast(m, r2, c=False):
    m = np.asarray(m, dtype=bool)
    return (_edt(~m, c) > np.uint32(r2)) & box(m.shape, radius(r2))


def open_fast(m, r2, c=False):
    return dilate_fast(erode_fast(m, r2, c), r2, c)


def close_fast(m, r2, c=False):
    R = radius(r2)
    return crop(erode_fast(dilate_fast(np.pad(np.asarray(m, dtype=bool), R), r2, c), r2, c), R)


def seal_fast(m, r2, c=False):
    m = np.asarray(m, dtype=bool)
    P = radius(r2) + 1
    d = dilate_fast(np.pad(m, P), r2, c)
    f = d | solid_ref.interior_cells(d)
    return m | crop(erode_fast(f, r2, c), P)


def apply_fast(op, m, r2, c=False):
    return (dilate_fast, erode_fast, open_fast, close_fast)[op](m, r2, c)
