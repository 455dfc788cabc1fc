"""CPU tests of the multi-hit reference (tests/multihit_ref.py): slot 0 of its lists is the pinned brute force's first hit, and its own
ordering, cursor and padding rules hold on hand-made lists."""
import numpy as np
import pytest

import multihit_ref as mr
import oracle
import vx_scenes

F = np.float32


def axis_rays(bmin, bmax, vs):
    """axis-parallel rays (two zero components) through the box, in both directions along every axis"""
    rays = []
    c = (np.asarray(bmin, np.float64) + np.asarray(bmax, np.float64)) / 2
    for a in range(3):
        for sgn in (1.0, -1.0):
            for off in (0.0, 0.37 * float(vs)):
                o = c + off
                o[a] = (bmin[a] - 1.0) if sgn > 0 else (bmax[a] + 1.0)
                d = np.zeros(3)
                d[a] = sgn
                rays.append(np.concatenate([o, d]))
    return np.array(rays, F)


@pytest.mark.parametrize("name,vs", [("rotcube", 0.21), ("cube", 0.25)])
def test_slot0_is_the_brute_force_first_hit(name, vs):
    v, t = vx_scenes.scene(name)
    vs = F(vs)
    words, _, gi = oracle.build_bool(v, t, vs)
    aabbs = oracle.bool_aabbs(words, gi, vs)
    assert len(aabbs) > 20
    rays = np.concatenate([vx_scenes.random_rays(300, gi["bmin"], gi["bmax"], seed=11), axis_rays(gi["bmin"], gi["bmax"], vs)])
    times = mr.hit_times(aabbs, rays)
    pos = np.sort(times[times > 0])
    window = (float(pos[int(0.4 * len(pos))]), float(pos[int(0.6 * len(pos))]))   # cuts the lists in the middle
    for tmin, tmax in ((0.001, 10000.0), window):
        bt, bp = oracle.trace_brute(aabbs, rays, tmin=tmin, tmax=tmax)
        for k in (1, 5):
            mt, mp, cnt = mr.select(times, k, tmin=tmin, tmax=tmax)
            assert np.array_equal(mt[:, 0].view(np.uint32), bt.view(np.uint32))
            assert np.array_equal(mp[:, 0], bp)
            assert np.array_equal(cnt > 0, bt > 0)
    assert (mr.select(times, 1)[2] > 1).any()


def test_order_cursor_and_padding():
    # four boxes in a row along x, the middle two coincide: a tie in t that prim breaks
    mn = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [4, 0, 0]], F)
    aabbs = np.zeros(4, oracle.AABB)
    aabbs["mn"], aabbs["mx"] = mn, mn + F(1)
    rays = np.array([[-1, 0.5, 0.5, 1, 0, 0], [6, 0.5, 0.5, -1, 0, 0], [-1, 5, 5, 1, 0, 0]], F)
    t, p, c = mr.multi(aabbs, rays, 3)
    assert c.tolist() == [4, 4, 0]
    assert t[0].tolist() == [1, 3, 3] and p[0].tolist() == [0, 1, 2]
    assert t[1].tolist() == [1, 3, 3] and p[1].tolist() == [3, 1, 2]      # against list order: the tie still goes to the smaller prim
    assert (t[2] == -1).all() and (p[2] == mr.NONE).all()
    # the cursor is strict in (t, prim): after (3, 1) come (3, 2) and the last box
    t, p, c = mr.multi(aabbs, rays, 3, after=(np.array([3, 3, -1], F), np.array([1, 2, 7], np.uint32)))
    assert c.tolist() == [2, 1, 0]
    assert t[0].tolist() == [3, 5, -1] and p[0].tolist() == [2, 3, 0xFFFFFFFF]
    assert t[1].tolist() == [5, -1, -1] and p[1].tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF]
    # a window and a per-ray tmax cut the list; the bounds are inclusive
    t, p, c = mr.multi(aabbs, rays, 2, tmin=3.0, tmax_per_ray=np.array([3, 10, 10], F))
    assert c.tolist() == [2, 3, 0] and t[0].tolist() == [3, 3] and t[1].tolist() == [3, 3]
