"""Reference for the multi-hit ray query on the octree (vx_octree_trace_multi*): tests/multihit_ref.py's brute force over the octree's AABB
list with every item but the first of each run of equal Morton codes struck out -- a run is one voxel and its prim is the first list index
of the run (include/voxhip.h).  Also the scenes the CPU and the GPU tests share.  A helper, not a test itself."""
import functools

import numpy as np

import multihit_ref as mr
import vx_scenes

F = np.float32
# (scene, voxel size): duplicates in all of them, lists longer than 32 in the second and third, 10 items per voxel in the last
SCENES = (("cube", 0.25), ("cube", 0.0625), ("rotcube", 0.09), ("adversarial", 0.1))
TIE = ("tie", 0.3)


def first_of_runs(items):
    """bool per list entry: the first item of its run of equal codes"""
    items = np.asarray(items, np.uint64)
    if not len(items):
        return np.zeros(0, bool)
    return np.r_[True, items[1:] != items[:-1]]


def hit_times(aabbs, items, rays):
    """multihit_ref.hit_times over the list, -1 on every entry that is not the first of its run"""
    times = mr.hit_times(aabbs, rays)
    times[:, ~first_of_runs(items)] = F(-1)
    return times


def multi(aabbs, items, rays, k, **kw):
    return mr.select(hit_times(aabbs, items, rays), k, **kw)


def multi_blocked(aabbs, items, rays, k, block=16, chunk=8):
    """multi() for long lists, a few rays at a time: the [rays, items] matrix of times never exists whole.  Also returns the counts the
    list would give with every duplicate counted -> (t, prim, count), count_with_duplicates"""
    first = first_of_runs(items)
    out, dup = [], []
    for s in range(0, len(rays), block):
        times = mr.hit_times(aabbs, rays[s:s + block], chunk=chunk)
        dup.append(mr.select(times, 1)[2])
        times[:, ~first] = F(-1)
        out.append(mr.select(times, k))
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3)), np.concatenate(dup)


def decode(items):
    """(x, y, z) of Morton codes, 21 bits per axis -> int64 [n, 3]"""
    m = np.asarray(items, np.uint64)
    out = np.zeros((len(m), 3), np.int64)
    for a in range(3):
        v = np.zeros(len(m), np.uint64)
        for b in range(21):
            v |= ((m >> np.uint64(3 * b + a)) & np.uint64(1)) << np.uint64(b)
        out[:, a] = v.astype(np.int64)
    return out


def tie_mesh():
    """Eight horizontal quads (z constant) through the cell centres of an 8^3 block of voxel size 0.3 with min corner (0.7, 2.3, -5.1), each
    inset by 0.05 voxels in x and y.  The lattice of such a grid is not exact in float32: the boxes of neighbouring cells overlap by a few
    ulps at some planes, and a ray inside such an overlap enters both cells at one t -- the ties only prim can order.  (The octree's own
    grid starts at the mesh's min corner: 8 x 8 x 7 cells, the quads on its lattice planes in z.)"""
    vs, n = 0.3, 8
    org = np.array([0.7, 2.3, -5.1])
    e = 0.05 * vs
    x0, x1 = org[0] + e, org[0] + n * vs - e
    y0, y1 = org[1] + e, org[1] + n * vs - e
    v, t = [], []
    for k in range(n):
        z = org[2] + (k + 0.5) * vs
        b = len(v)
        v += [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
        t += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    return np.array(v, F), np.array(t, np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    return tie_mesh() if name == "tie" else vx_scenes.scene(name)
