"""The scenes and ray batches of the mesh multi-hit tests (tests/test_mesh_multihit_cpu.py checks them against the conditions they must
meet, tests/test_gpu_mesh_multihit.py runs them): each the smallest in which one mechanism of the query can fail.  Every case and its
reference hits are built once and left unchanged.  A helper for the tests, not a test itself."""
import functools

import numpy as np

import instance_ref
import mesh_multihit_ref as mm
import vx_scenes
from test_gpu_mesh_trace import floor_scene, grazing_floor_rays, ray_families, vertex_rays

F = np.float32
BVH_CASES = ("cube", "layers", "floor", "adversarial", "blob")
NLAYERS = 40
ILL_SIN = 1.0 / 1024.0   # vx_bvh.hip's kIllSin: triangles below it are on the BVH's side list


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64)], axis=1), F)


def axis_rays_at(points, axis, lo, hi):
    """rays along +axis and -axis through the given (u, v) points, u and v the two axes after `axis` cyclically; exact arithmetic"""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    out = []
    for sgn, start in ((1.0, lo - 2.0), (-1.0, hi + 2.0)):
        o = np.zeros((len(points), 3))
        o[:, u], o[:, v], o[:, axis] = points[:, 0], points[:, 1], start
        d = np.zeros((len(points), 3))
        d[:, axis] = sgn
        out.append(_rays(o, d))
    return np.concatenate(out)


def cube_rays():
    """at the faces' diagonals (one of the two is the shared edge of the face's triangles: two prims at one t), at edge midpoints and edge
    points (two faces), at the vertices (up to six triangles), along every axis; then the vertex / edge family from outside and random rays"""
    c = np.linspace(-0.875, 0.875, 8)
    pts = np.concatenate([np.stack([c, c], 1), np.stack([c, -c], 1), np.stack([np.ones(8), c], 1), np.stack([c, -np.ones(8)], 1),
                          np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [1, 0], [0, -1], [0.3, 0.1]], np.float64)])
    v, t = vx_scenes.cube()
    return np.concatenate([axis_rays_at(pts, a, -1.0, 1.0) for a in range(3)] + [vertex_rays(v, t, 400, 5), vx_scenes.random_rays(300, v.min(0), v.max(0), seed=6)])


def layers_scene():
    """NLAYERS parallel quads of two triangles each, 0.25 apart along z"""
    V, T = [], []
    for k in range(NLAYERS):
        z = 0.25 * k
        n = len(V)
        V += [(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)]
        T += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
    return np.array(V, F), np.array(T, np.int32)


def layers_rays():
    """along z off the quads' diagonal (one triangle per layer) and on it (both, at one t), slanted through the stack, and random"""
    c = np.linspace(-0.75, 0.75, 7)
    pts = np.concatenate([np.stack([c, 0.5 * c + 0.125], 1), np.stack([c, c], 1)])
    v, _ = layers_scene()
    rng = np.random.default_rng(8)
    n = 150
    a = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.full((n, 1), -1.0)], 1)
    b = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.full((n, 1), 11.0)], 1)
    d = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
    return np.concatenate([axis_rays_at(pts, 2, 0.0, 0.25 * (NLAYERS - 1)), _rays(a, d), _rays(b, -d), vx_scenes.random_rays(200, v.min(0), v.max(0), seed=9)])


def side_listed(v, t):
    """the triangles vx_bvh.hip puts on its side list: the sine of the angle at v0 at most ILL_SIN, both edges non-zero (float64, its formula)"""
    p = np.asarray(v, F).astype(np.float64)[np.asarray(t).reshape(-1, 3)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    c = np.cross(e1, e2)
    l1, l2 = (e1 * e1).sum(1), (e2 * e2).sum(1)
    return (l1 > 0) & (l2 > 0) & ((c * c).sum(1) <= ILL_SIN * ILL_SIN * l1 * l2)


def adversarial_rays(v, t):
    """at points of the side-listed (collinear, sliver) triangles from many directions -- their Moeller-Trumbore is rounding noise that
    accepts now and then -- and random rays through the rest"""
    rng = np.random.default_rng(10)
    ill = np.flatnonzero(side_listed(v, t))
    k = ill[rng.integers(0, len(ill), 1500)]
    p = v[t[k]].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), len(k))
    tgt = (p * w[:, :, None]).sum(1)
    d = rng.normal(size=(len(k), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (tgt - 3.0 * d).astype(F)
    dr = tgt - o.astype(np.float64)
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    return np.concatenate([_rays(o, dr), vx_scenes.random_rays(800, v.min(0), v.max(0), seed=11)])


class Case:
    pass


@functools.lru_cache(maxsize=None)
def bvh_case(name):
    """mesh, rays and the reference hits of the default interval"""
    c = Case()
    c.name = name
    c.max_leaf = (0,)
    if name == "cube":
        c.v, c.t = vx_scenes.cube()
        c.rays = cube_rays()
    elif name == "layers":
        c.v, c.t = layers_scene()
        c.rays = layers_rays()
    elif name == "floor":
        c.v, c.t = floor_scene()
        c.rays = np.concatenate([grazing_floor_rays(600, 12), vx_scenes.random_rays(300, c.v.min(0), c.v.max(0), seed=13)])
    elif name == "adversarial":
        c.v, c.t = vx_scenes.scene("adversarial")
        c.rays = adversarial_rays(c.v, c.t)
    elif name == "blob":
        c.v, c.t = vx_scenes.blob(nlon=52, nlat=48)   # 4888 triangles
        c.rays = np.concatenate(list(ray_families(c.v, c.t, 300, 14).values()))
        c.max_leaf = (1, 4)
    else:
        raise KeyError(name)
    c.hits = mm.all_hits(c.v, c.t, c.rays)
    return c


@functools.lru_cache(maxsize=None)
def tlas_case():
    """Two BLAS (the cube, a small blob) and six instances: rotation with non-uniform scale, shear, two instances of the blob under ONE
    transform (every hit ties across them), a masked-out instance, a small cube inside the blobs' box."""
    c = Case()
    cube = vx_scenes.cube()
    blob = vx_scenes.blob(nlon=26, nlat=22)   # 1092 triangles
    c.meshes = [cube, blob]
    rng = np.random.default_rng(21)
    twin = instance_ref.transform(rot=instance_ref.random_rotation(rng), scale=(1.0, 0.8, 1.2), shear=0.3, offset=(2.5, 0.5, 0.0))
    tr = [instance_ref.transform(rot=instance_ref.random_rotation(rng), scale=(1.5, 0.5, 1.0), offset=(-2.0, 0.0, 0.5)),
          twin, twin,
          instance_ref.transform(offset=(0.0, 3.0, 0.0)),
          instance_ref.transform(rot=instance_ref.random_rotation(rng), scale=(0.2, 0.2, 0.3), offset=(2.5, 0.5, 0.0)),
          instance_ref.transform(rot=instance_ref.random_rotation(rng), scale=(0.7, 1.1, 0.9), shear=-0.4, offset=(0.0, -2.5, 1.0))]
    c.inst = instance_ref.make_instances(tr, blas=[0, 1, 1, 0, 0, 1], mask=[0xFF, 0xFF, 0xFF, 0, 0xFF, 0xFF])
    world = np.concatenate([instance_ref.world_vertices(c.inst["transform"][i], c.meshes[int(c.inst["blas"][i])][0]) for i in range(len(tr))])
    lo, hi = world.min(0), world.max(0)
    # random rays through the scene, rays at world vertices of the instances (shared edges and vertices of their meshes), rays starting inside
    idx = rng.integers(0, len(world), 500)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (world[idx].astype(np.float64) - 12.0 * d).astype(F)
    dr = world[idx].astype(np.float64) - o.astype(np.float64)
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    inside = _rays(np.tile([[2.5, 0.5, 0.0]], (100, 1)) + rng.uniform(-0.05, 0.05, (100, 3)), d[:100])
    c.rays = np.concatenate([vx_scenes.random_rays(900, lo, hi, seed=22), _rays(o, dr), inside])
    c.hits = mm.all_hits_tlas(c.meshes, c.inst, c.rays)
    return c


def equal_t_runs(sel, field):
    """per ray: does its list hold two neighbouring entries of bit-equal t that differ in `field`"""
    t = sel["t"]
    same = (t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0)
    return (same & (sel[field][:, 1:] != sel[field][:, :-1])).any(axis=1)
