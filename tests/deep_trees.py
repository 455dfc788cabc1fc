"""Scenes whose radix trees are chains, stacks of coincident hits, and the instruments that show a ray really holds `height` stack entries
there.  A helper for tests/test_deep_trees_cpu.py and tests/test_gpu_deep_trees.py, not a test itself (the regime: DESIGN.md sections 6c
and 6e; the stack the trace kernels size to the build's height: the heads of vx_bvh.hip and vx_tlas.hip).

Every scene, ray batch and reference result is cached per process and read-only: the tests of a module share one copy.

Units: u = 1/1024 of the unit box, one cell of the builds' 10-bit Morton quantisation per axis.  The chain's bounding-box centres sit at
cell centres (q + 0.5) u, so no rounding of the builds' float32 arithmetic moves a key."""
import functools
import types

import numpy as np

import instance_ref
import mesh_multihit_ref
import mesh_ref
import vx_scenes

F = np.float32
U = 1.0 / 1024.0
LEAF = 0x80000000
NODE = np.dtype([("mn", np.float32, 3), ("a", np.uint32), ("mx", np.float32, 3), ("b", np.uint32)])   # voxhip.BVH_NODE
CLUSTERS = (1, 64, 4096)
PURE_CHAIN_N = (2, 3, 4, 5, 8)
STACK_MARGIN = 3            # a deep ray holds at least height - 3 entries (the worst the CPU model of the scene showed)
# the constants of the builds this module restates
K_BOX_EXT, K_BOX_POS = F(1.0 / 1024.0), F(1.0 / 262144.0)                                  # vx_bvh.hip: bvh_pad
K_COND, K_CORNER, K_EXT = F(1.0 / 65536.0), F(1.0 / 262144.0), F(1.0 / 1024.0)            # vx_tlas.hip: k_tlas_prep


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
def chain_q():
    """the 25 quantised centres: (256, 256, 256), then for i = 1..8 the z, the y, the x component set to 512 - 2^(8 - i)"""
    q = [256, 256, 256]
    out = [tuple(q)]
    for i in range(1, 9):
        for axis in (2, 1, 0):
            q[axis] = 512 - 2 ** (8 - i)
            out.append(tuple(q))
    return np.array(out, np.int64)


def _equilateral(box_centre, box_half):
    """triangles perpendicular to (1, 1, 1) with bounding box box_centre +- box_half: A = c + h (2, -1, -1), B = c + h (-1, 2, -1),
    C = c + h (-1, -1, 2), whose box is c + h [-1, 2]^3 -> float64 [n, 3, 3]"""
    ctr = np.asarray(box_centre, np.float64).reshape(-1, 3)
    h = (np.asarray(box_half, np.float64) / 1.5).reshape(-1, 1, 1)
    c = ctr[:, None, :] - 0.5 * h
    return c + h * np.array([[2.0, -1.0, -1.0], [-1.0, 2.0, -1.0], [-1.0, -1.0, 2.0]])[None]


PINS = np.array([[[0, 0, 0], [1, 1, 0], [0, 1, 1]], [[1, 1, 1], [0, 0, 1], [1, 0, 0]]], np.float64)   # each spans [0, 1]^3


@functools.lru_cache(maxsize=None)
def chain_scene(m, mirrored=False):
    """Two pins spanning [0, 1]^3 (triangles 0, 1), the 25 chain triangles (2..26), and a cluster of m triangles sharing the centre
    (511.5 u)^3 with box half-sizes from 0.1 u to 0.4 u (27..).  Vertices are not shared.  -> ns(v, t, m, mirrored, name)

    mirrored: the point reflection x -> 1 - x of it (before rounding): the chain then converges on the centre from above, the cluster
    shares the cell (512, 512, 512) of the pins, every split isolates the HIGHEST key, and the pins are a pair at the deep end of the
    chain and not a leaf pair beside the root.  In the scene as it stands the root's near child holds the pins, so a diagonal ray has
    popped its first entry before it goes down the chain and holds at most height - 1; in the mirrored scene (rays mirrored too) it
    holds one entry for every interior node of the longest path: at m = 1 exactly `height` of them."""
    ctr = (chain_q() + 0.5) * U
    half = 0.75 * np.abs(ctr - 0.5).max(axis=1)
    cl_ctr = np.full((m, 3), 511.5 * U)
    cl_half = np.linspace(0.1 * U, 0.4 * U, m)
    tri = np.concatenate([PINS, _equilateral(ctr, half), _equilateral(cl_ctr, cl_half)])
    if mirrored:
        tri = 1.0 - tri
    v = tri.reshape(-1, 3).astype(F)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return _ns(v=_frozen(v), t=_frozen(t), m=m, mirrored=mirrored, name="chain%d%s" % (m, "m" if mirrored else ""))


@functools.lru_cache(maxsize=None)
def stacked_scene(copies):
    """one well-conditioned triangle `copies` times (separate vertex triples, identical coordinates: 0 .. copies-1), and the same again one
    unit further along -z (copies .. 2 copies - 1) -> ns(v, t, copies, rays)"""
    one = np.array([[-1.0, -0.75, 0.0], [1.25, -0.5, 0.0], [0.0, 1.0, 0.0]])
    far = one + np.array([0.0, 0.0, -1.0])
    v = np.concatenate([np.tile(one, (copies, 1)), np.tile(far, (copies, 1))]).astype(F)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    rng = np.random.default_rng(41)
    n = 96
    o = np.stack([rng.uniform(-0.3, 0.4, n), rng.uniform(-0.3, 0.3, n), np.full(n, 2.0)], 1)
    d = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n), np.full(n, -1.0)], 1)
    miss = np.array([[3.0, 3.0, 2.0, 0.0, 0.0, -1.0], [0.0, 0.0, -3.0, 0.0, 0.0, -1.0]])           # beside and behind both layers
    rays = np.concatenate([np.concatenate([o, d], 1), miss]).astype(F)
    return _ns(v=_frozen(v), t=_frozen(t), copies=copies, rays=_frozen(rays), name="stacked%d" % copies)


# ---- the builds' keys, restated ----------------------------------------------------------------------------------------------------------
def spread10(q):
    """bit i of q (i < 10) -> bit 3 i"""
    q = np.asarray(q, np.uint64)
    out = np.zeros_like(q)
    for i in range(10):
        out |= ((q >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def _quantise(c, lo, hi):
    """k_bvh_keys / k_tlas_keys in float32: (c - lo) / ext * 1024, clamped to 0 .. 1023 (NaN and a flat axis -> 0), then the code"""
    c, lo, hi = np.asarray(c, F), np.asarray(lo, F), np.asarray(hi, F)
    ext = hi - lo
    with np.errstate(all="ignore"):
        f = np.where(ext > 0, (c - lo) / ext * F(1024.0), F(0))
    q = np.where(f >= F(1023.0), 1023, np.where(f > 0, np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), 0)).astype(np.uint64)
    return spread10(q[:, 0]) | (spread10(q[:, 1]) << np.uint64(1)) | (spread10(q[:, 2]) << np.uint64(2))


def bvh_keys(v, t):
    """k_bvh_keys in numpy float32: the bounds centre (min + max) * 0.5 over the union of the bounds, key = code << 32 | triangle"""
    p = np.asarray(v, F)[np.asarray(t, np.int64).reshape(-1, 3)]
    mn, mx = p.min(axis=1), p.max(axis=1)
    code = _quantise((mn + mx) * F(0.5), mn.min(axis=0), mx.max(axis=0))
    return (code << np.uint64(32)) | np.arange(len(p), dtype=np.uint64)


def bvh_pad(v, t):
    """vx_bvh.hip's bvh_pad of a mesh: 2^-10 of the root box's largest side + 2^-18 of its largest |coordinate| (+ 1e-30)"""
    p = np.asarray(v, F)[np.asarray(t, np.int64).reshape(-1)]
    mn, mx = p.min(axis=0), p.max(axis=0)
    return (K_BOX_EXT * (mx - mn).max() + K_BOX_POS * np.abs(np.concatenate([mn, mx])).max()) + F(1e-30)


def instance_boxes(meshes, inst):
    """k_tlas_prep's widened world box of every instance in numpy float32 -> (lo [n, 3], hi [n, 3]); an inactive instance: +inf / -inf.
    The margins are restated to a few ulps (the instances of this module sit at cell centres, far from where an ulp moves a key)."""
    n = len(inst)
    lo, hi = np.full((n, 3), np.inf, F), np.full((n, 3), -np.inf, F)
    w, _ = instance_ref.inverse(inst["transform"])
    act = instance_ref.active(inst, [len(np.asarray(tr).reshape(-1, 3)) for _, tr in meshes])
    for i in np.flatnonzero(act):
        vv, tr = meshes[int(inst["blas"][i])]
        p = np.asarray(vv, F)[np.asarray(tr, np.int64).reshape(-1)]
        pad = bvh_pad(vv, tr)
        blo, bhi = p.min(axis=0) - pad, p.max(axis=0) + pad
        corners = np.array([[(bhi if c >> a & 1 else blo)[a] for a in range(3)] for c in range(8)], F)
        m = inst["transform"][i].astype(F)
        wc = instance_ref.world_vertices(m, corners)
        bmin, bmax = wc.min(axis=0), wc.max(axis=0)
        a3 = np.abs(m.reshape(3, 4)[:, :3])
        nm = ((a3[:, 0] + a3[:, 1]) + a3[:, 2]).max()
        aw = np.abs(w[i].reshape(3, 4)[:, :3])
        nw = ((aw[:, 0] + aw[:, 1]) + aw[:, 2]).max()
        cond = min(nm * nw, F(3.0e38))
        tn = np.abs(m.reshape(3, 4)[:, 3]).max()
        cmax = max(np.abs(bmin).max(), np.abs(bmax).max())
        margin = (K_COND * cond * (tn + cmax) + K_CORNER * (nm * np.abs(corners).max() + tn)) + K_EXT * (bmax - bmin).max()
        lo[i], hi[i] = bmin - margin, bmax + margin
    return lo, hi


def tlas_keys(meshes, inst):
    """k_tlas_keys: the widened world box's centre over the union of the active boxes, key = code << 32 | instance"""
    lo, hi = instance_boxes(meshes, inst)
    fin = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1)
    with np.errstate(all="ignore"):
        code = _quantise((lo + hi) * F(0.5), lo[fin].min(axis=0), hi[fin].max(axis=0))
    return (code << np.uint64(32)) | np.arange(len(inst), dtype=np.uint64)


# ---- the radix tree ------------------------------------------------------------------------------------------------------------------------
def _split(k, lo, hi):
    """first index of [lo, hi] whose key has the highest bit set in which k[lo] and k[hi] differ"""
    bit = int(k[lo] ^ k[hi]).bit_length() - 1
    return lo + int(np.searchsorted((k[lo:hi + 1] >> np.uint64(bit)) & np.uint64(1), 1))


def radix_height(keys):
    """the height (interior nodes on the longest root-to-leaf path) of the radix tree over the sorted unique keys, which splits every
    range at the highest differing bit (k_bvh_karras)"""
    k = np.sort(np.asarray(keys, np.uint64))
    assert len(k) == 0 or np.all(k[1:] != k[:-1])
    best, todo = 0, [(0, len(k) - 1, 0)]
    while todo:
        lo, hi, d = todo.pop()
        if lo >= hi:
            best = max(best, d)
            continue
        s = _split(k, lo, hi)
        todo += [(lo, s - 1, d + 1), (s, hi, d + 1)]
    return best


def radix_nodes(keys, mn, mx):
    """the radix tree as a node array in the library's layout (root at 0; interior: a, b = children; leaf: a = the item of the key's low
    32 bits, b = LEAF | 1), boxes the exact min / max below; mn, mx [n, 3] per item"""
    keys = np.asarray(keys, np.uint64)
    order = np.argsort(keys)
    k = keys[order]
    item = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    n = len(k)
    nodes = np.zeros(2 * n - 1, NODE)
    nxt = [1]

    def build(idx, lo, hi):
        if lo == hi:
            nodes[idx] = (mn[item[lo]], item[lo], mx[item[lo]], LEAF | 1)
            return
        s = _split(k, lo, hi)
        a, b = nxt[0], nxt[0] + 1
        nxt[0] += 2
        build(a, lo, s - 1)
        build(b, s, hi)
        nodes[idx] = (np.minimum(nodes["mn"][a], nodes["mn"][b]), a, np.maximum(nodes["mx"][a], nodes["mx"][b]), b)

    build(0, 0, n - 1)
    return nodes


def scene_radix_nodes(sc):
    p = sc.v[sc.t.astype(np.int64)]
    return radix_nodes(bvh_keys(sc.v, sc.t), p.min(axis=1), p.max(axis=1))


def node_depth(nodes):
    """the largest number of interior nodes above a leaf"""
    best, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        if int(nodes["b"][i]) & LEAF:
            best = max(best, d)
        else:
            todo += [(int(nodes["a"][i]), d + 1), (int(nodes["b"][i]), d + 1)]
    return best


def is_chain(nodes):
    """every interior node has a leaf child"""
    leaf = (nodes["b"] & np.uint32(LEAF)) != 0
    inner = np.flatnonzero(~leaf)
    return bool(np.all(leaf[nodes["a"][inner]] | leaf[nodes["b"][inner]]))


# ---- the stack a ray holds -------------------------------------------------------------------------------------------------------------------
def _entry(tree, i, o, inv, deg):
    """entry time of the ray into the exact box of node i in float64, None when it passes it (or the box is empty)"""
    lo, hi = tree[0][i], tree[1][i]
    t0, t1 = -INF, INF
    for a in (0, 1, 2):
        if lo[a] > hi[a]:
            return None
        if deg[a]:
            if not lo[a] <= o[a] <= hi[a]:
                return None
            continue
        p, q = (lo[a] - o[a]) * inv[a], (hi[a] - o[a]) * inv[a]
        if p > q:
            p, q = q, p
        if p > t0:
            t0 = p
        if q < t1:
            t1 = q
    return t0 if t0 <= t1 and t1 >= 0.0 else None


INF = float("inf")


def as_tree(nodes):
    """a node array as Python lists (the model walks thousands of nodes per ray): (lo, hi, a, b)"""
    if isinstance(nodes, tuple):
        return nodes
    return (nodes["mn"].astype(np.float64).tolist(), nodes["mx"].astype(np.float64).tolist(), nodes["a"].tolist(), nodes["b"].tolist())


def stack_model(nodes, ray, left_on_tie=True, clamp=False):
    """The descent order at the head of vx_bvh.hip replayed on a node array (the library's, or radix_nodes'): the nearer child first,
    the farther one pushed when the ray crosses it too, nothing pruned (the count query's regime), on the exact boxes in float64 (the
    kernels' boxes are wider: they cross at least these).  left_on_tie: which child counts as nearer on equal entry times; clamp: entry
    times below 0 count as 0.  -> the largest number of entries held.  An instrument for the coverage of an input, never the oracle of
    a result."""
    tree = as_tree(nodes)
    ray = [float(x) for x in np.asarray(ray, np.float64)]
    o, d = ray[:3], ray[3:]
    deg = [x == 0.0 for x in d]
    inv = [0.0 if x == 0.0 else 1.0 / x for x in d]
    if len(tree[2]) == 0 or _entry(tree, 0, o, inv, deg) is None:
        return 0
    held, stack, cur = 0, [], 0
    while True:
        if not tree[3][cur] & LEAF:
            a, b = tree[2][cur], tree[3][cur]
            ta, tb = _entry(tree, a, o, inv, deg), _entry(tree, b, o, inv, deg)
            if ta is not None and tb is not None:
                if clamp:
                    ta, tb = max(ta, 0.0), max(tb, 0.0)
                near_a = ta <= tb if left_on_tie else ta < tb
                stack.append(b if near_a else a)
                held = max(held, len(stack))
                cur = a if near_a else b
                continue
            if ta is not None or tb is not None:
                cur = a if ta is not None else b
                continue
        if not stack:
            return held
        cur = stack.pop()


def most_held(nodes, rays, **kw):
    tree = as_tree(nodes)
    return max(stack_model(tree, r, **kw) for r in rays)


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------
N_DIAGONAL = 48
DIAGONAL = slice(0, N_DIAGONAL)                       # of deep_rays: the rays that hold the stack
REVERSED = slice(N_DIAGONAL, 2 * N_DIAGONAL)


def _diagonal(seed, target=(0.0, 0.0, 0.0), scale=1.0):
    """rays from (1.2, 1.2, 1.2) along (-1, -1, -1) with 1e-4 jitter of the origin (every second one: of the direction too); ray 0 exact"""
    rng = np.random.default_rng(seed)
    o = 1.2 + rng.uniform(-1e-4, 1e-4, (N_DIAGONAL, 3))
    d = -1.0 + rng.uniform(-1e-4, 1e-4, (N_DIAGONAL, 3)) * (np.arange(N_DIAGONAL) % 2)[:, None]
    o[0], d[0] = 1.2, -1.0
    return np.concatenate([np.asarray(target) + scale * o, d], axis=1)


@functools.lru_cache(maxsize=None)
def deep_rays(m, mirrored=False):
    """the rays of chain_scene(m): the jittered diagonal rays (DIAGONAL), the same reversed (from behind the box, REVERSED), 32 rays from
    inside the cluster, 200 random rays over the box; mirrored: origins 1 - o, directions -d (before rounding)"""
    rng = np.random.default_rng(100 + m)
    dia = _diagonal(7)
    rev = dia.copy()
    rev[:, :3] = dia[:, :3] + 1.4 * dia[:, 3:]       # (-0.2, -0.2, -0.2), beyond the box
    rev[:, 3:] = -dia[:, 3:]
    n = 32
    ins_o = 511.5 * U + rng.uniform(-0.3 * U, 0.3 * U, (n, 3))
    ins_d = rng.normal(size=(n, 3))
    ins_d[: n // 2] = np.where(np.arange(n // 2)[:, None] % 2 == 0, -1.0, 1.0) + rng.uniform(-0.05, 0.05, (n // 2, 3))   # along the diagonal, both ways
    ins_d /= np.linalg.norm(ins_d, axis=1, keepdims=True)
    rnd = vx_scenes.random_rays(200, F([0, 0, 0]), F([1, 1, 1]), seed=11 + m)
    rays = np.concatenate([dia, rev, np.concatenate([ins_o, ins_d], 1), rnd.astype(np.float64)])
    if mirrored:
        rays = np.concatenate([1.0 - rays[:, :3], -rays[:, 3:]], axis=1)
    return _frozen(rays.astype(F))


# ---- instances ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unit_triangle():
    """the one-triangle BLAS: perpendicular to (1, 1, 1), box [-1, 2]^3"""
    return _frozen(F([[2, -1, -1], [-1, 2, -1], [-1, -1, 2]])), _frozen(np.int32([[0, 1, 2]]))


def _scaled(s, offset):
    return instance_ref.transform(np.eye(3), (s, s, s), 0.0, offset)


def _box_transforms(mesh, ctr, half, mirror=False):
    """scale + translation that put the mesh's box (a cube) at ctr +- half; mirror: the scale negated (a point reflection)"""
    v, t = mesh
    p = np.asarray(v, np.float64)[np.asarray(t).reshape(-1)]
    bc, bh = (p.min(0) + p.max(0)) / 2, (p.max(0) - p.min(0)).max() / 2
    sign = -1.0 if mirror else 1.0
    return [_scaled(sign * h / bh, c - (sign * h / bh) * bc) for c, h in zip(np.asarray(ctr, np.float64).reshape(-1, 3), np.asarray(half, np.float64).reshape(-1))]


@functools.lru_cache(maxsize=None)
def chain_instances(tall):
    """Two pin instances, three cells wide in the low and the high corner of [0, 1]^3 (0: as is, 1: mirrored; a pin over the whole box
    would have its centre on the edge between cells 511 and 512, where the margins' rounding decides), and 25 chain instances whose
    widened world boxes have their centres at the cells chain_q() of the pins' union and 0.75 of the largest distance from 0.5 as
    half-size.  The low pin's key lies below the chain and is isolated like the chain's: 27 instances, height 26 = n - 1.  tall: the BLAS
    is chain_scene(4096)'s mesh (height 38), else the one triangle.  -> ns(meshes, inst, rays)"""
    sc = chain_scene(4096)
    mesh = (sc.v, sc.t) if tall else unit_triangle()
    pins = _box_transforms(mesh, [1.5 * U] * 3, [1.5 * U]) + _box_transforms(mesh, [1.0 - 1.5 * U] * 3, [1.5 * U], mirror=True)
    plo, phi = instance_boxes([mesh], instance_ref.make_instances(pins))
    lo, ext = plo.min(0).astype(np.float64), (phi.max(0).astype(np.float64) - plo.min(0))
    ctr = lo + (chain_q() + 0.5) / 1024.0 * ext
    half = 0.75 * np.abs(ctr - 0.5).max(axis=1)
    inst = instance_ref.make_instances(pins + _box_transforms(mesh, ctr, half))
    assert np.array_equal(tlas_keys([mesh], inst) >> np.uint64(32), _quantise_q(np.concatenate([[[1] * 3, [1022] * 3], chain_q()])))
    rays = np.concatenate([deep_rays(1)[: 2 * N_DIAGONAL], vx_scenes.random_rays(100 if tall else 200, F([0, 0, 0]), F([1, 1, 1]), seed=23)])
    inst.setflags(write=False)
    return _ns(meshes=[mesh], inst=inst, rays=_frozen(rays.astype(F)), tall=tall)


def _quantise_q(q):
    q = np.asarray(q, np.uint64)
    return spread10(q[:, 0]) | (spread10(q[:, 1]) << np.uint64(1)) | (spread10(q[:, 2]) << np.uint64(2))


@functools.lru_cache(maxsize=None)
def pure_chain_instances(n):
    """n instances of the one triangle and no pins, their boxes one cell wide on the diagonal at cells 0, 512, 768, ... (1024 - 2^(10 - k))
    and, the last, 1023: every split of the radix tree isolates the lowest key, so its height is n - 1 -> ns(meshes, inst, rays)"""
    q = np.array([1024 - 2 ** (10 - k) for k in range(n - 1)] + [1023], np.float64)
    ctr = np.repeat(((q + 0.5) * U)[:, None], 3, axis=1)
    inst = instance_ref.make_instances(_box_transforms(unit_triangle(), ctr, np.full(n, 0.5 * U)))
    inst.setflags(write=False)
    rays = np.concatenate([_diagonal(9), vx_scenes.random_rays(100, F([0, 0, 0]), F([1, 1, 1]), seed=29)])
    return _ns(meshes=[unit_triangle()], inst=inst, rays=_frozen(rays.astype(F)))


def instance_radix_nodes(meshes, inst):
    lo, hi = instance_boxes(meshes, inst)
    return radix_nodes(tlas_keys(meshes, inst), lo, hi)


@functools.lru_cache(maxsize=None)
def coincident_instances(n):
    """n instances of the one triangle under one and the same transform -> ns(meshes, inst, rays): every hit is an n-fold tie"""
    tr = instance_ref.transform(instance_ref.random_rotation(np.random.default_rng(5)), (0.5, 0.75, 0.5), 0.0, (0.25, -0.5, 0.125))
    inst = instance_ref.make_instances([tr] * n)
    inst.setflags(write=False)
    w = instance_ref.world_vertices(tr, unit_triangle()[0])
    rays = vx_scenes.random_rays(96, w.min(0), w.max(0), seed=31)
    return _ns(meshes=[unit_triangle()], inst=inst, rays=_frozen(rays.astype(F)))


@functools.lru_cache(maxsize=None)
def random_instances(n):
    """n random rigid-and-scaled transforms of the one triangle inside the unit box"""
    rng = np.random.default_rng(37)
    tr = [instance_ref.transform(instance_ref.random_rotation(rng), rng.uniform(0.02, 0.1, 3), 0.0, rng.uniform(0.1, 0.9, 3)) for _ in range(n)]
    inst = instance_ref.make_instances(tr)
    inst.setflags(write=False)
    return inst


def tlas_height_bound(n):
    """vx_tlas.hip's tlas_height_bound"""
    if n <= 1:
        return 0
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(n - 1, 30 + lg)


# ---- references, computed once ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_closest(m, mirrored=False):
    sc = chain_scene(m, mirrored)
    return tuple(_frozen(a) for a in mesh_ref.closest(sc.v, sc.t, deep_rays(m, mirrored)))


@functools.lru_cache(maxsize=None)
def chain_hits(m, mirrored=False):
    sc = chain_scene(m, mirrored)
    return mesh_multihit_ref.all_hits(sc.v, sc.t, deep_rays(m, mirrored))


@functools.lru_cache(maxsize=None)
def chain_tmax(m, mirrored=False):
    """per ray: the t of the middle hit of its full list (10 where it has none)"""
    h = chain_hits(m, mirrored)
    cnt = np.bincount(h.ray, minlength=h.n)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    out = np.full(h.n, 10.0, F)
    have = cnt > 0
    out[have] = h.t[(start + cnt // 2)[have]]
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def stacked_hits(copies):
    sc = stacked_scene(copies)
    return mesh_multihit_ref.all_hits(sc.v, sc.t, sc.rays)


def ill_conditioned(v, t):
    """the side-list criterion of k_bvh_bounds in float64: the sine of the angle at v0 below 2^-10"""
    p = np.asarray(v, F)[np.asarray(t, np.int64).reshape(-1, 3)].astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    c = np.cross(e1, e2)
    l1, l2 = (e1 * e1).sum(1), (e2 * e2).sum(1)
    return (l1 > 0) & (l2 > 0) & ((c * c).sum(1) <= 2.0 ** -20 * l1 * l2)
