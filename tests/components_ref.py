"""Numpy restatement of connected-component labelling (vx_grid_components*, vx_grid_component_stats), for the tests.

M = the occupied cells of the bitmask.  Two cells of M are adjacent under 6-connectivity when they share a face, under 26-connectivity when
they share a face, an edge or a corner; nothing wraps.  Labels: 0 for empty cells, 1..K for cells of M, the components numbered in
ascending order of their smallest cell index i = x + X*(y + Y*z).  Record k - 1 of the statistics describes label k: its cell count and
its inclusive cell bounds (x, y, z).

`label` is hook-and-jump union-find: every occupied cell starts as its own root; each round hooks, for every pair of adjacent occupied
cells (the 3 or 13 forward offsets), the larger of the two roots to the smaller, then jumps pointers until every cell points at its root.
Rounds run until no pair has two roots.  `label_c` is the same labelling by a sequential union-find in plain C (tests/components_ref.c,
built with the host compiler on first use): fast enough for 512^3; a CPU test pins it to the numpy form.  No scipy.
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from solid_ref import pack, unpack  # noqa: F401  (the bitmask layout: i = x + X*(y + Y*z), LSB first)

COMPONENT = np.dtype([("cells", "<u8"), ("min", "<u4", 3), ("max", "<u4", 3)])  # vx_component


def forward_offsets(connectivity):
    """the neighbour offsets (dz, dy, dx) that point to a larger cell index: 3 for 6-connectivity, 13 for 26."""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                if connectivity == 6 and abs(dz) + abs(dy) + abs(dx) != 1:
                    continue
                out.append((dz, dy, dx))
    assert connectivity in (6, 26) and len(out) == (3 if connectivity == 6 else 13)
    return out


def _pairs(m, connectivity):
    """(a, b): the cell indices of every adjacent occupied pair, b = a + a forward offset."""
    Z, Y, X = m.shape
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    A, B = [], []
    for dz, dy, dx in forward_offsets(connectivity):
        src = tuple(slice(max(0, -d), n - max(0, d)) for d, n in ((dz, Z), (dy, Y), (dx, X)))
        dst = tuple(slice(max(0, d), n - max(0, -d)) for d, n in ((dz, Z), (dy, Y), (dx, X)))
        both = m[src] & m[dst]
        A.append(idx[src][both])
        B.append(idx[dst][both])
    return np.concatenate(A), np.concatenate(B)


def number(m, root):
    """labels from the root of every cell (root[i] = the smallest cell of i's component): roots numbered in ascending order."""
    flat = np.asarray(m, dtype=bool).reshape(-1)
    is_root = flat & (root == np.arange(flat.size))
    rank = np.cumsum(is_root, dtype=np.int64)  # rank[r] = the label of root r
    lab = np.where(flat, rank[np.where(flat, root, 0)], 0)
    return lab.astype(np.uint32).reshape(m.shape), int(is_root.sum())


def label(cells, connectivity=6):
    """bool[Z, Y, X] -> (uint32[Z, Y, X] labels, K), by hook-and-jump."""
    m = np.asarray(cells, dtype=bool)
    p = np.arange(m.size, dtype=np.int64)
    a, b = _pairs(m, connectivity)
    while True:
        ra, rb = p[a], p[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        sel = lo != hi
        if not sel.any():
            break
        np.minimum.at(p, hi[sel], lo[sel])  # hi is a root (p is flat): link it to the smallest root it touches
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    return number(m, p)


_LIB = None


def _c_lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "components_ref.c")
        tag = hashlib.sha1(open(src, "rb").read()).hexdigest()[:12]
        d = os.path.join(tempfile.gettempdir(), "voxhip_components_ref_%d" % os.getuid())
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "components_ref_%s.so" % tag)
        if not os.path.exists(so):
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", tmp, src])
            os.replace(tmp, so)
        L = ctypes.CDLL(so)
        L.label.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
        L.label.restype = ctypes.c_int64
        _LIB = L
    return _LIB


def label_c(cells, connectivity=6):
    """label by the C helper (sequential union-find)."""
    t = np.ascontiguousarray(cells, dtype=np.uint8)
    Z, Y, X = t.shape
    out = np.zeros(t.shape, dtype=np.uint32)
    if not t.size:
        return out, 0
    k = _c_lib().label(t.ctypes.data, out.ctypes.data, X, Y, Z, connectivity)
    if k < 0:
        raise MemoryError("components_ref.c: out of memory")
    return out, int(k)


def components(words, dim, connectivity=6, fast=False):
    """the bitmask `words` of a grid of `dim` = (X, Y, Z) -> (labels uint32[Z, Y, X], K)."""
    m = unpack(words, dim)
    return (label_c if fast else label)(m, connectivity)


def stats(labels, k):
    """COMPONENT[k] from the labels: per label its cell count and inclusive (x, y, z) bounds."""
    out = np.zeros(k, dtype=COMPONENT)
    if not k:
        return out
    Z, Y, X = labels.shape
    lab = labels.reshape(-1)
    occ = np.flatnonzero(lab)
    L = lab[occ]
    order = np.argsort(L, kind="stable")
    L, c = L[order], occ[order]
    starts = np.flatnonzero(np.r_[True, L[1:] != L[:-1]])
    assert len(starts) == k and L[starts[0]] == 1 and L[starts[-1]] == k
    out["cells"] = np.diff(np.r_[starts, len(L)])
    for a, v in enumerate((c % X, (c // X) % Y, c // (X * Y))):
        out["min"][:, a] = np.minimum.reduceat(v, starts)
        out["max"][:, a] = np.maximum.reduceat(v, starts)
    return out


def brute_stats(labels, k):
    """the statistics one label at a time: for small grids."""
    out = np.zeros(k, dtype=COMPONENT)
    for j in range(1, k + 1):
        z, y, x = np.nonzero(labels == j)
        out[j - 1]["cells"] = len(x)
        out[j - 1]["min"] = (x.min(), y.min(), z.min())
        out[j - 1]["max"] = (x.max(), y.max(), z.max())
    return out
