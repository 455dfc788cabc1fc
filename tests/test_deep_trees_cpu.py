"""The inputs of tests/test_gpu_deep_trees.py, checked without a device: the chain scenes really have radix trees as tall as claimed, a
diagonal ray really holds (nearly) `height` stack entries in them, the cluster really overflows K = 32, the stacked scene really ties 100
hits at one t, and nothing in them is on the build's side list.  Properties of the helper and of the brute-force references alone."""
import numpy as np
import pytest

import deep_trees as dt
import instance_ref
import mesh_multihit_ref

# radix height of chain_scene(m, mirrored) (2 pins, 25 chain triangles, m in the cluster) and the most stack entries one of its diagonal
# rays holds, as the restated build and the descent model give them.  As the scene stands, the root's near child is the pair of pins and the
# ray has popped that entry before it walks the chain: it holds at most height - 1.  Mirrored, the pins end the chain, and at m = 1 the
# ray holds `height` entries, one for every interior node above its deepest leaf -- the only rays a stack one level short shows on.
HEIGHT = {(1, False): 26, (64, False): 32, (4096, False): 38, (1, True): 26, (64, True): 31, (4096, True): 37}
HELD = {(1, False): 25, (64, False): 29, (4096, False): 36, (1, True): 26, (64, True): 30, (4096, True): 36}
ISSUE_FLOOR = {1: 24, 64: 30, 4096: 36}
SCENES = [(m, mirrored) for mirrored in (False, True) for m in dt.CLUSTERS]
TLAS_CHAIN_HEIGHT = 26        # 27 instances: the bound's n - 1 branch, reached


def test_chain_q_is_a_chain_of_keys():
    q = dt.chain_q()
    assert len(q) == 25 and tuple(q[0]) == (256, 256, 256) and tuple(q[-1]) == (511, 511, 511)
    code = dt._quantise_q(q)
    assert np.all(code[1:] > code[:-1])                       # ascending: z, then y, then x move up
    nodes = dt.radix_nodes((code << np.uint64(32)) | np.arange(25, dtype=np.uint64), np.zeros((25, 3)), np.ones((25, 3)))
    assert dt.is_chain(nodes) and dt.node_depth(nodes) == 24


@pytest.mark.parametrize("m,mirrored", SCENES)
def test_chain_scene_height(m, mirrored):
    sc = dt.chain_scene(m, mirrored)
    assert len(sc.t) == 27 + m and len(sc.v) == 3 * len(sc.t)
    p = sc.v[sc.t]
    assert np.array_equal(p.reshape(-1, 3).min(0), [0, 0, 0]) and np.array_equal(p.reshape(-1, 3).max(0), [1, 1, 1])
    keys = dt.bvh_keys(sc.v, sc.t)
    # every chain triangle sits in the cell the scene is built around, the cluster in the last one
    q = np.concatenate([[[512] * 3] * 2, dt.chain_q(), [[511] * 3] * m])
    q[2:] = 1023 - q[2:] if mirrored else q[2:]
    assert np.array_equal(keys >> np.uint64(32), dt._quantise_q(q))
    h = dt.radix_height(keys)
    assert h == HEIGHT[m, mirrored] and h >= ISSUE_FLOOR[m]
    assert dt.node_depth(dt.scene_radix_nodes(sc)) == h


@pytest.mark.parametrize("m,mirrored", SCENES)
@pytest.mark.parametrize("left_on_tie", [True, False])
def test_chain_scene_holds_the_stack(m, mirrored, left_on_tie):
    sc = dt.chain_scene(m, mirrored)
    tree = dt.as_tree(dt.scene_radix_nodes(sc))
    rays = dt.deep_rays(m, mirrored)
    H = HEIGHT[m, mirrored]
    for clamp in (False, True):
        held = dt.most_held(tree, rays[dt.DIAGONAL][:6], left_on_tie=left_on_tie, clamp=clamp)
        assert H - dt.STACK_MARGIN <= held <= H, (held, clamp)
        if not clamp:
            assert held == HELD[m, mirrored]
    other = dt.most_held(tree, rays[dt.REVERSED][:6], left_on_tie=left_on_tie)
    if mirrored:    # the pins lie in the deep end: every subtree above them spans the unit box and is entered first, whichever way the ray goes
        assert other >= H - dt.STACK_MARGIN
    else:           # the direction matters: the same rays sent the other way hold far fewer
        assert other < H - 2 * dt.STACK_MARGIN


def test_mirrored_chain_holds_the_whole_height():
    """one entry for every interior node of the longest path: on these rays a stack of height - 1 levels loses a subtree"""
    assert HELD[1, True] == HEIGHT[1, True] == 26
    for m in dt.CLUSTERS:
        assert HELD[m, True] >= HEIGHT[m, True] - 1 and HELD[m, False] <= HEIGHT[m, False] - 1


@pytest.mark.parametrize("mirrored", [False, True])
def test_cluster_overflows_k32(mirrored):
    h = dt.chain_hits(64, mirrored)
    cnt = np.bincount(h.ray, minlength=h.n)
    assert (cnt > 32).sum() >= 5 and cnt.max() >= 90
    big = dt.chain_hits(4096, mirrored)
    assert np.bincount(big.ray, minlength=big.n).max() > 3600
    # and a tmax in the middle of the chain cuts a list that is otherwise full
    tm = dt.chain_tmax(64, mirrored)
    sc = dt.chain_scene(64, mirrored)
    cut = mesh_multihit_ref.all_hits(sc.v, sc.t, dt.deep_rays(64, mirrored), tmax_per_ray=tm)
    c2 = np.bincount(cut.ray, minlength=cut.n)
    assert np.all(c2 <= cnt) and (c2[dt.DIAGONAL] < cnt[dt.DIAGONAL]).all() and (c2[dt.DIAGONAL] >= 5).all()


def test_stacked_scene_ties_100():
    sc = dt.stacked_scene(100)
    assert len(sc.t) == 200 and np.array_equal(sc.v[sc.t[0]], sc.v[sc.t[99]]) and not np.array_equal(sc.v[sc.t[0]], sc.v[sc.t[100]])
    h = dt.stacked_hits(100)
    cnt = np.bincount(h.ray, minlength=h.n)
    assert (cnt == 200).sum() >= 90 and set(np.unique(cnt)) == {0, 200}
    for r in np.flatnonzero(cnt == 200)[:20]:
        t, prim = h.t[h.ray == r], h.prim[h.ray == r]
        assert len(np.unique(t.view(np.uint32))) == 2 and t[0] == t[99] and t[100] == t[199] and t[99] < t[100]    # two runs of 100 bit-equal t
        assert np.array_equal(prim, np.arange(200))


def test_no_scene_triangle_is_on_the_side_list():
    for m, mirrored in SCENES:
        sc = dt.chain_scene(m, mirrored)
        assert not dt.ill_conditioned(sc.v, sc.t).any()
    sc = dt.stacked_scene(100)
    assert not dt.ill_conditioned(sc.v, sc.t).any()
    assert not dt.ill_conditioned(*dt.unit_triangle()).any()
    # the smallest cluster triangle is well resolved in float32: its edges are thousands of ulps of its coordinates long
    sc = dt.chain_scene(4096)
    p = sc.v[sc.t[27]].astype(np.float64)
    assert np.linalg.norm(p[1] - p[0]) > 2000 * np.spacing(np.float32(0.5))


def test_tlas_height_bound_restated():
    def formula(n):       # the head of vx_tlas.hip: min(n - 1, 30 + ceil(log2 n)), 0 for fewer than two instances
        return 0 if n <= 1 else min(n - 1, 30 + (n - 1).bit_length())
    ns = list(range(41)) + [2 ** k for k in range(6, 32)] + [2 ** k + 1 for k in range(6, 31)]
    for n in ns:
        assert dt.tlas_height_bound(n) == formula(n), n
    assert all(dt.tlas_height_bound(n) == n - 1 for n in range(1, 36)) and dt.tlas_height_bound(36) == 35 and dt.tlas_height_bound(37) == 36
    assert dt.tlas_height_bound(38) == 36 and dt.tlas_height_bound(2 ** 31 - 1) == 61


@pytest.mark.parametrize("tall", [False, True])
def test_chain_instances_reach_the_bound(tall):
    ci = dt.chain_instances(tall)
    n = len(ci.inst)
    assert n == 27 and instance_ref.active(ci.inst, [len(ci.meshes[0][1])]).all()
    nodes = dt.instance_radix_nodes(ci.meshes, ci.inst)
    h = dt.radix_height(dt.tlas_keys(ci.meshes, ci.inst))
    assert h == TLAS_CHAIN_HEIGHT == dt.tlas_height_bound(n) == dt.node_depth(nodes) and dt.is_chain(nodes)
    for left in (True, False):
        assert dt.most_held(nodes, ci.rays[dt.DIAGONAL][:6], left_on_tie=left) >= h - dt.STACK_MARGIN
    # every chain box lies inside the pins' union, so the pins alone fix the quantisation
    lo, hi = dt.instance_boxes(ci.meshes, ci.inst)
    assert np.all(lo[2:] > lo[:2].min(0)) and np.all(hi[2:] < hi[:2].max(0))


@pytest.mark.parametrize("n", dt.PURE_CHAIN_N)
def test_pure_chain_instances(n):
    pc = dt.pure_chain_instances(n)
    assert len(pc.inst) == n
    keys = dt.tlas_keys(pc.meshes, pc.inst)
    nodes = dt.instance_radix_nodes(pc.meshes, pc.inst)
    assert len(np.unique(keys >> np.uint64(32))) == n                  # distinct codes: the index bits take no part
    assert dt.radix_height(keys) == n - 1 == dt.tlas_height_bound(n) and dt.is_chain(nodes)
    assert dt.most_held(nodes, pc.rays[dt.DIAGONAL][:6]) == n - 1      # the diagonal crosses every box: the full stack


def test_coincident_instances_tie():
    co = dt.coincident_instances(64)
    h = mesh_multihit_ref.all_hits_tlas(co.meshes, co.inst, co.rays)
    cnt = np.bincount(h.ray, minlength=h.n)
    assert set(np.unique(cnt)) == {0, 64} and (cnt == 64).sum() >= 30
    r = int(np.flatnonzero(cnt == 64)[0])
    assert len(np.unique(h.t[h.ray == r].view(np.uint32))) == 1 and np.array_equal(h.inst[h.ray == r], np.arange(64))


def test_helper_arrays_are_read_only():
    sc = dt.chain_scene(1)
    for a in (sc.v, sc.t, dt.deep_rays(1), dt.stacked_scene(100).rays, dt.chain_instances(False).inst, dt.chain_closest(1)[0]):
        assert not a.flags.writeable
    assert dt.chain_scene(1) is sc
