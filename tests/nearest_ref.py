"""Numpy restatement of the feature transform (vx_grid_nearest), for the tests.

T = the target cells (the occupied cells of the bitmask, or the empty ones).  i(c) = x + X*(y + Y*z).
N(c) = min { i(o) : o in T, |c - o|^2 = min over T of |c - p|^2 }: the nearest target, the smallest index (smallest z, then y, then x) among
equally near ones; N(c) = i(c) on T; 0xFFFFFFFF everywhere when T is empty.

`brute` is the definition itself, every pair of cells, `argmin` over the targets in ascending index order: for tiny grids.  `nearest` is
separable: along x the nearer of the last and the next target of the row, the left one on a tie; along y and z the minimum over the column
of (i - j)^2 + g(j), one shift j at a time in ascending order with a strict `<`, so the smaller j keeps every tie, carrying the winner's
coordinates -- O(n N) per axis, plain and slow.  `nearest_c` is the same transform by the linear lower envelope in plain C
(tests/nearest_ref.c, built with the host compiler on first use); a CPU test pins the three to each other.  No scipy.
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from solid_ref import pack, unpack  # noqa: F401  (the bitmask layout: i = x + X*(y + Y*z), LSB first)

SENTINEL = 0xFFFFFFFF
_BIG = np.int64(1) << 40  # larger than any squared distance of a grid within the 32-bit limit


def brute(target):
    """the definition: bool[Z, Y, X] -> uint32[Z, Y, X]."""
    target = np.asarray(target, dtype=bool)
    Z, Y, X = target.shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    cz, cy, cx = zz.reshape(-1), yy.reshape(-1), xx.reshape(-1)
    idx = np.flatnonzero(target.reshape(-1))  # ascending cell index
    if not idx.size:
        return np.full(target.shape, SENTINEL, dtype=np.uint32)
    d = (cz[:, None] - cz[None, idx]) ** 2 + (cy[:, None] - cy[None, idx]) ** 2 + (cx[:, None] - cx[None, idx]) ** 2
    return idx[np.argmin(d, axis=1)].astype(np.uint32).reshape(target.shape)  # (argmin: the first, so the smallest index, of the minima)


def _x_pass(target):
    """(g, x'): squared distance along x to the nearest target of the row and its position, left on a tie (int64; _BIG / -1: none)."""
    idx = np.broadcast_to(np.arange(target.shape[2], dtype=np.int64), target.shape)
    left = np.maximum.accumulate(np.where(target, idx, -_BIG), axis=2)
    right = np.flip(np.minimum.accumulate(np.flip(np.where(target, idx, 2 * _BIG), axis=2), axis=2), axis=2)
    dl, dr = idx - left, right - idx
    d = np.where(dl <= dr, dl, dr)
    fx = np.where(dl <= dr, left, right)
    none = d >= _BIG
    return np.where(none, _BIG, d * d), np.where(none, -1, fx)


def _axis_pass(g, feats, axis):
    """min over j of (i - j)^2 + g[j] along `axis`, the smallest such j, and `feats` taken at that j -> (g', feats', j)."""
    a = np.moveaxis(g, axis, -1)
    fs = [np.moveaxis(f, axis, -1) for f in feats]
    n = a.shape[-1]
    i = np.arange(n, dtype=np.int64)
    best = np.full(a.shape, _BIG, dtype=np.int64)
    bj = np.full(a.shape, -1, dtype=np.int64)
    bf = [np.full(a.shape, -1, dtype=np.int64) for _ in fs]
    for j in range(n):
        gj = a[..., j:j + 1]
        cand = np.where(gj >= _BIG, _BIG, gj + (i - j) ** 2)
        take = cand < best  # strict: an earlier j keeps a tie
        best = np.where(take, cand, best)
        bj = np.where(take, j, bj)
        bf = [np.where(take, f[..., j:j + 1], b) for f, b in zip(fs, bf)]
    back = lambda v: np.moveaxis(v, -1, axis)  # noqa: E731
    return back(best), [back(b) for b in bf], back(bj)


def nearest(target):
    """bool[Z, Y, X] targets -> uint32[Z, Y, X]: N(c), SENTINEL when there is no target."""
    target = np.asarray(target, dtype=bool)
    Z, Y, X = target.shape
    g, fx = _x_pass(target)
    g, (fx,), fy = _axis_pass(g, [fx], 1)
    g, (fx, fy), fz = _axis_pass(g, [fx, fy], 0)
    return np.where(g >= _BIG, SENTINEL, fx + X * (fy + Y * fz)).astype(np.uint32)


_LIB = None


def _c_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nearest_ref.c")
        tag = hashlib.sha1(open(src, "rb").read()).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), "voxhip_nearest_ref_%d" % os.getuid())
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "nearest_ref_%s.so" % tag)
        if not os.path.exists(so):
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", tmp, src])
            os.replace(tmp, so)
        L = ctypes.CDLL(so)
        L.nearest.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.nearest.restype = ctypes.c_int
        _LIB = L
    return _LIB


def nearest_c(target):
    """nearest by the C helper (linear lower envelope per column)."""
    t = np.ascontiguousarray(target, dtype=np.uint8)
    Z, Y, X = t.shape
    out = np.empty(t.shape, dtype=np.uint32)
    if t.size and _c_lib().nearest(t.ctypes.data, out.ctypes.data, X, Y, Z) != 0:
        raise MemoryError("nearest_ref.c: out of memory")
    return out


def dist_sq_of(n):
    """|c - N(c)|^2 per cell from a field of nearest indices uint32[Z, Y, X]; SENTINEL where N is the sentinel."""
    Z, Y, X = n.shape
    if not n.size:
        return np.zeros(n.shape, np.uint32)
    zz, yy, xx = np.meshgrid(np.arange(Z, dtype=np.int64), np.arange(Y, dtype=np.int64), np.arange(X, dtype=np.int64), indexing="ij")
    i = n.astype(np.int64)
    d = (xx - i % X) ** 2 + (yy - i // X % Y) ** 2 + (zz - i // (X * Y)) ** 2
    return np.where(n == SENTINEL, SENTINEL, d).astype(np.uint32)


def gather(n, values, fill):
    """values[N(c)] per cell, `fill` at the sentinel."""
    v = np.asarray(values, dtype=np.uint32).reshape(-1)
    if not v.size:
        return np.zeros(n.shape, np.uint32)
    safe = np.where(n == SENTINEL, 0, n)
    return np.where(n == SENTINEL, np.uint32(fill), v[safe]).astype(np.uint32)
