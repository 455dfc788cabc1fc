"""CPU tests of the multi-hit query on the octree.  The reference of the GPU tests (tests/octree_multihit_ref.py: the brute force over the
de-duplicated list) is checked here against the oracle's own octree, so that what tests/test_gpu_octree_multihit.py takes for granted is a
fact: slot 0 is the first-hit brute force over the FULL list, counts and t sequences are the Bool grid's, and the inputs hold duplicates,
lists longer than 32 and ties.  The entry points are exported and refuse null arguments before anything touches a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import multihit_ref as mr
import octree_multihit_ref as om
import vx_scenes
from test_gpu_multihit import family_rays

F = np.float32
INVALID_ARG = 1
# scene -> (items, runs, largest count, rays with more than 32 hits) on 600 vx_scenes.random_rays, seed 3
FIGURES = {("cube", 0.25): (258, 169, 14, 0), ("cube", 0.0625): (3354, 2977, 37, 2), ("rotcube", 0.09): (5022, 4307, 35, 2),
           ("adversarial", 0.1): (10731, 997, 25, 0)}


@functools.lru_cache(maxsize=None)
def built(name, vs):
    import oracle
    v, t = om.mesh(name)
    oc = oracle.octree(v, t, F(vs))
    words, _, gi = oracle.build_bool(v, t, F(vs))
    return oc, words, gi


@pytest.mark.parametrize("name,vs", om.SCENES)
def test_reference_against_the_oracle(name, vs):
    import oracle
    oc, words, gi = built(name, vs)
    rays = vx_scenes.random_rays(600, gi["bmin"], gi["bmax"], seed=3)
    t, p, c = om.multi(oc["aabbs"], oc["items"], rays, 32)
    # the inputs: duplicates, and overflow of K = 32 where the table says so
    first = om.first_of_runs(oc["items"])
    assert (len(oc["items"]), int(first.sum()), int(c.max()), int((c > 32).sum())) == FIGURES[(name, vs)]
    assert first.sum() < len(first)
    # slot 0 is the first-hit query's brute force over the full list, duplicates included
    bt, bp = oracle.trace_brute(oc["aabbs"], rays)
    assert np.array_equal(t[:, 0].view(np.uint32), bt.view(np.uint32)) and np.array_equal(p[:, 0], bp)
    assert (bt > 0).mean() > 0.02
    # every listed prim is the first index of its run
    assert first[p[p != mr.NONE]].all()
    # the distinct boxes are the Bool grid's: the same counts and the same t sequences
    gt, _, gc = mr.multi(oracle.bool_aabbs(words, gi, F(vs)), rays, 32)
    assert np.array_equal(c, gc) and np.array_equal(t.view(np.uint32), gt.view(np.uint32))


def test_tie_scene_ties():
    """Rays of the tie scene carry several voxels at bit-equal t, and prim ascends inside every tie"""
    import oracle
    name, vs = om.TIE
    oc, _, gi = built(name, vs)
    assert gi["dim"] == (8, 8, 7)
    occ = np.unique(om.decode(oc["items"]), axis=0)
    rays = family_rays(gi["dim"], oc["root_min"], F(vs), occ, seed=5)
    t, p, c = om.multi(oc["aabbs"], oc["items"], rays, 32)
    tie = (t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0)
    assert (tie.sum(axis=1) >= 4).sum() >= 8
    assert (p[:, 1:] > p[:, :-1])[tie].all()
    assert len(oc["items"]) > om.first_of_runs(oc["items"]).sum()
    bt, bp = oracle.trace_brute(oc["aabbs"], rays)
    assert np.array_equal(t[:, 0].view(np.uint32), bt.view(np.uint32)) and np.array_equal(p[:, 0], bp)


def test_octree_multihit_symbols_exported(vx):
    L = C.CDLL(vx.LIB_PATH)
    for n in ("vx_octree_trace_multi", "vx_octree_trace_multi_device"):
        assert hasattr(L, n) and n in vx.SYMBOLS
    assert hasattr(vx.Octree, "trace_multi") and hasattr(vx.Octree, "trace_multi_device")


def test_octree_multihit_null_handle_and_args(vx):
    L = vx.lib()
    rays = np.zeros((4, 6), F)
    t = np.full((4, 2), F(7), F)
    a = vx.MultiHitArgs()
    a.base.rays, a.base.num_rays, a.base.t, a.max_hits = rays.ctypes.data, 4, t.ctypes.data, 2
    for fn in (L.vx_octree_trace_multi, L.vx_octree_trace_multi_device):
        assert fn(None, C.byref(a)) == INVALID_ARG
        assert fn(None, None) == INVALID_ARG
    assert b"null" in L.vx_last_error()
    assert (t == F(7)).all()
