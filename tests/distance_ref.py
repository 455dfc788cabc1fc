"""Numpy restatement of the distance fields (vx_grid_distance_sq, vx_grid_sdf), for the tests.

M = the occupied cells of the bitmask.  D_out(c) = min over o in M of |c - o|^2 (cell units, exact integers), 0xFFFFFFFF when M is empty;
D_in(c) = the same over the empty cells, 0xFFFFFFFF when there is none.  s(c) = vs * sqrt((float32)D_out(c)) off M and
-(vs * sqrt((float32)D_in(c))) on M, all in float32, the sentinel giving +-inf.

`edt_sq` is separable: along x the distance to the nearest target of the row (from running indices), then along y and z the exact
minimum over the column of (i - j)^2 + g(j), one shift j at a time -- O(n N) per axis, plain and slow.  `edt_sq_c` is the same
transform by the linear lower envelope of parabolas in plain C (tests/distance_ref.c, built with the host compiler on first use):
fast enough for 512^3; a CPU test pins it to the numpy form.  No scipy.
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


def _axis_pass(g, axis):
    """min over j of (i - j)^2 + g[j] along `axis` (int64, _BIG = no target)."""
    a = np.moveaxis(g, axis, -1)
    n = a.shape[-1]
    i = np.arange(n, dtype=np.int64)
    out = np.full(a.shape, _BIG, dtype=np.int64)
    for j in range(n):
        gj = a[..., j:j + 1]
        cand = np.where(gj >= _BIG, _BIG, gj + (i - j) ** 2)
        np.minimum(out, cand, out=out)
    return np.moveaxis(out, -1, axis)


def _x_pass(target):
    """squared distance along x to the nearest target cell of the row (int64, _BIG = none)."""
    Z, Y, X = target.shape
    idx = np.broadcast_to(np.arange(X, dtype=np.int64), target.shape)
    left = np.maximum.accumulate(np.where(target, idx, -_BIG), axis=2)
    right = np.flip(np.minimum.accumulate(np.flip(np.where(target, idx, 2 * _BIG), axis=2), axis=2), axis=2)
    d = np.minimum(idx - left, right - idx)
    return np.where(d >= _BIG, _BIG, d * d)


def edt_sq(target):
    """bool[Z, Y, X] targets -> uint32[Z, Y, X]: the exact squared distance to the nearest target, SENTINEL when there is none."""
    target = np.asarray(target, dtype=bool)
    g = _x_pass(target)
    g = _axis_pass(g, 1)
    g = _axis_pass(g, 0)
    return np.where(g >= _BIG, SENTINEL, g).astype(np.uint32)


_LIB = None


def _c_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "distance_ref.c")
        tag = hashlib.sha1(open(src, "rb").read()).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), "voxhip_distance_ref_%d" % os.getuid())
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "distance_ref_%s.so" % tag)
        if not os.path.exists(so):
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", tmp, src])
            os.replace(tmp, so)
        L = ctypes.CDLL(so)
        L.edt_sq.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.edt_sq.restype = ctypes.c_int
        _LIB = L
    return _LIB


def edt_sq_c(target):
    """edt_sq by the C helper (linear lower envelope per column)."""
    t = np.ascontiguousarray(target, dtype=np.uint8)
    Z, Y, X = t.shape
    out = np.empty(t.shape, dtype=np.uint32)
    if t.size and _c_lib().edt_sq(t.ctypes.data, out.ctypes.data, X, Y, Z) != 0:
        raise MemoryError("distance_ref.c: out of memory")
    return out


def _cells(words, dim):
    return unpack(words, dim)


def distance_sq(words, dim, inside=False, fast=False):
    """the bitmask `words` of a grid of `dim` = (X, Y, Z) -> D_out (inside=False) or D_in, uint32[Z, Y, X]."""
    m = _cells(words, dim)
    f = edt_sq_c if fast else edt_sq
    return f(~m if inside else m)


def sdf_from(m, d_out, d_in, vs):
    """s from the mask and both squared fields, in float32 exactly as the contract writes it."""
    vs = np.float32(vs)
    with np.errstate(over="ignore"):
        so = vs * np.sqrt(d_out.astype(np.float32))
        si = -(vs * np.sqrt(d_in.astype(np.float32)))
    so = np.where(d_out == SENTINEL, np.float32(np.inf), so).astype(np.float32)
    si = np.where(d_in == SENTINEL, np.float32(-np.inf), si).astype(np.float32)
    return np.where(m, si, so).astype(np.float32)


def sdf(words, dim, vs, fast=False):
    """the signed field of the bitmask, float32[Z, Y, X]."""
    m = _cells(words, dim)
    f = edt_sq_c if fast else edt_sq
    return sdf_from(m, f(m), f(~m), vs)


def brute_sq(target):
    """the definition itself, every pair of cells: for tiny grids."""
    target = np.asarray(target, dtype=bool)
    Z, Y, X = target.shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    cz, cy, cx = zz.reshape(-1), yy.reshape(-1), xx.reshape(-1)
    t = target.reshape(-1)
    if not t.any():
        return np.full(target.shape, SENTINEL, dtype=np.uint32)
    d = (cz[:, None] - cz[None, t]) ** 2 + (cy[:, None] - cy[None, t]) ** 2 + (cx[:, None] - cx[None, t]) ** 2
    return d.min(axis=1).astype(np.uint32).reshape(target.shape)
