#!/usr/bin/env python3
"""What k_voxelize's sweep costs on the large triangles of a scene, counted on the CPU (numpy and vx_scenes only; no GPU): voxel tests and
64-lane sweep turns per large triangle as built (every voxel of an alive row's work units) and with each unit cut to the exact real-valued
x interval of its row's plane test, rounded outwards to whole voxels and widened by one voxel on each side -- the bound that sat_row_interval (csrc/vx_math.h) approaches.
usage: row_interval_estimate.py [scene [grid [min_units]]]      (defaults: atrium262k 512 4096)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd"))
import vx_scenes  # noqa: E402

F = np.float32


def centre(org, vs, i):
    """cell_centre: org + (i + 0.5f) * vs in float32"""
    return (org + ((i.astype(F) + F(0.5)) * vs)).astype(F)


def ranges(v3, org, vs, dim):
    """cand_axis (serial driver: vsize = half * 2) + trim_axis for one axis of every triangle -> start, end"""
    half = F(vs * F(0.5))
    vsize = F(half * F(2.0))
    tmn, tmx = v3.min(axis=1), v3.max(axis=1)
    s = np.maximum(((tmn - org) / vsize).astype(np.int64), 0)
    e = np.minimum(((tmx - org) / vsize).astype(np.int64) + 2, dim)

    def sep(i):
        p = v3 - centre(org, vs, np.maximum(i, 0))[:, None]
        return (p.min(axis=1) > half) | (p.max(axis=1) < -half)
    while True:
        m = (e > s) & sep(e - 1)
        if not m.any():
            break
        e = e - m
    while True:
        m = (e > s) & sep(s)
        if not m.any():
            break
        s = s + m
    return s, np.maximum(e, s)


def rows_alive(v, cy, cz, h):
    """sat_row_setup<EPS = true>: the x-invariant tests of rows (cy, cz) of one triangle, in float32"""
    py = [F(v[3 * k + 1]) - cy for k in range(3)]
    pz = [F(v[3 * k + 2]) - cz for k in range(3)]
    sep = (np.minimum.reduce(py) > h) | (np.maximum.reduce(py) < -h) | (np.minimum.reduce(pz) > h) | (np.maximum.reduce(pz) < -h)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ey, ez = py[b] - py[a], pz[b] - pz[a]
        R = h * np.abs(ez) + h * np.abs(ey)
        live = ~((np.abs(ez) + np.abs(ey)) < F(1e-8))
        d = [(-(py[k] * ez)) + pz[k] * ey for k in range(3)]
        sep |= live & ((np.minimum.reduce(d) > R) | (np.maximum.reduce(d) < -R))
    return ~sep


def plane_interval(v, cy, cz, org, vs):
    """the exact (float64) interval of voxel indices x whose centre passes the plane test of row (cy, cz) -> lo, hi (reals)"""
    p = np.asarray(v, np.float64).reshape(3, 3)
    e0, e1 = p[1] - p[0], p[2] - p[1]
    n = np.cross(e0, e1)
    h = 0.5 * float(vs)
    rr = h * np.abs(n).sum()
    k = n[1] * (p[0, 1] - cy.astype(np.float64)) + n[2] * (p[0, 2] - cz.astype(np.float64))
    if n[0] == 0.0:
        return np.full(cy.shape, -np.inf), np.full(cy.shape, np.inf)
    a, b = p[0, 0] + (k - rr) / n[0], p[0, 0] + (k + rr) / n[0]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return (lo - float(org)) / float(vs) - 0.5, (hi - float(org)) / float(vs) - 0.5


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "atrium262k"
    grid = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    min_units = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    verts, tris = vx_scenes.scene(scene)
    verts = np.ascontiguousarray(verts, F)
    bmin, bmax = verts.min(axis=0), verts.max(axis=0)
    vs = F(F(bmax.max() - bmin.min()) / F(grid)) if scene != "atrium262k" else F(32.0 / grid)
    dim = np.ceil((bmax - bmin) / vs).astype(np.int64)
    tv = verts[tris].reshape(-1, 9)
    s, e = zip(*[ranges(tv[:, a::3], bmin[a], vs, dim[a]) for a in range(3)])
    nx, ny, nz = (e[a] - s[a] for a in range(3))
    nseg = np.where(nx > 0, ((s[0] + nx - 1) >> 5) - (s[0] >> 5) + 1, 0)
    units = np.where((nx > 0) & (ny > 0) & (nz > 0), nseg * ny * nz, 0)
    base = np.concatenate([[0], np.cumsum(units)])
    print("%s at %s, voxel size %g: %d triangles, %d work units, %d wave passes" % (scene, "x".join(str(int(d)) for d in dim), vs, len(tv), base[-1], (base[-1] + 63) // 64))
    tot = np.zeros(6, np.int64)
    h = F(vs * F(0.5))
    print("%8s %18s %9s %10s %9s | %10s %9s   (hits need the plane interval: tests / turns with it +- 1 voxel)" % ("triangle", "box", "units", "tests", "turns", "tests", "turns"))
    for t in np.nonzero(units >= min_units)[0]:
        yy, zz = np.meshgrid(np.arange(s[1][t], e[1][t]), np.arange(s[2][t], e[2][t]), indexing="xy")   # row = z * ny + y
        yy, zz = yy.reshape(-1), zz.reshape(-1)
        cy, cz = centre(bmin[1], vs, yy), centre(bmin[2], vs, zz)
        alive = rows_alive(tv[t], cy, cz, h)
        lo, hi = plane_interval(tv[t], cy, cz, bmin[0], vs)
        x0r, x1r = int(s[0][t]), int(e[0][t])
        seg0 = x0r >> 5
        # units of the triangle in their order: row-major, segments of a row next to each other
        sx = np.arange(int(nseg[t]))
        x0 = np.maximum(x0r, (seg0 + sx) << 5)[None, :].repeat(len(yy), 0)
        x1 = np.minimum(x1r, (seg0 + sx + 1) << 5)[None, :].repeat(len(yy), 0)
        a = np.clip(np.floor(lo) - 1, x0r - 1, x1r + 1).astype(np.int64)[:, None]
        b = np.clip(np.ceil(hi) + 2, x0r - 1, x1r + 1).astype(np.int64)[:, None]
        n_built = np.where(alive[:, None], x1 - x0, 0).reshape(-1)
        c0, c1 = np.maximum(x0, a), np.minimum(x1, b)
        n_cut = np.where(alive[:, None], np.maximum(c1 - c0, 0), 0).reshape(-1)
        # wave passes: 64 consecutive units of the whole build's unit list
        pad = int(base[t] % 64)
        def turns(n):
            w = np.concatenate([np.zeros(pad, np.int64), n])
            w = np.concatenate([w, np.zeros((-len(w)) % 64, np.int64)])
            return int(w.reshape(-1, 64).max(axis=1).sum())
        r = (int(units[t]), int(n_built.sum()), turns(n_built), int(n_cut.sum()), turns(n_cut))
        print("%8d %18s %9d %10d %9d | %10d %9d" % ((t, "%dx%dx%d" % (nx[t], ny[t], nz[t])) + r))
        tot[:5] += r
        tot[5] += 1
    print("%8s %18s %9d %10d %9d | %10d %9d" % ("sum", "%d triangles" % tot[5], tot[0], tot[1], tot[2], tot[3], tot[4]))


if __name__ == "__main__":
    main()
