"""CPU tests of the mesh multi-hit reference (tests/mesh_multihit_ref.py) and of the inputs the GPU tests run (tests/mesh_multihit_cases.py):
slot 0 of the reference's lists is the pinned brute force's first hit, pages chained through the cursor give the unpaged list, the
inputs meet the conditions under which no GPU case passes vacuously, and the library and voxhip.py agree on the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_ref
import mesh_multihit_cases as mc
import mesh_multihit_ref as mm
import mesh_ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the reference against the first-hit brute force and against itself ----------------------------------------------------------------
@pytest.mark.parametrize("name", mc.BVH_CASES)
def test_slot0_is_the_first_hit_bvh(name):
    c = mc.bvh_case(name)
    pos = np.sort(c.hits.t)
    window = (float(pos[int(0.3 * len(pos))]), float(pos[int(0.7 * len(pos))]))
    for tmin, tmax in ((0.001, 10000.0), window):
        h = c.hits if tmax == 10000.0 else mm.all_hits(c.v, c.t, c.rays, tmin=tmin, tmax=tmax)
        rt, rp, rb = mesh_ref.closest(c.v, c.t, c.rays, tmin=tmin, tmax=tmax)
        for k in (1, 5):
            s = mm.select(h, k)
            assert np.array_equal(bits(s["t"][:, 0]), bits(rt)) and np.array_equal(s["prim"][:, 0], rp)
            assert np.array_equal(bits(s["bary"][:, 0]), bits(rb))
            assert np.array_equal(s["count"] > 0, rt > 0)
            assert not s["instance"][s["t"] > 0].any() and (s["instance"][s["t"] < 0] == mm.NONE).all()


def test_slot0_is_the_first_hit_tlas():
    c = mc.tlas_case()
    rt, ri, rp, rb = instance_ref.closest(c.meshes, c.inst, c.rays)
    s = mm.select(c.hits, 4)
    assert np.array_equal(bits(s["t"][:, 0]), bits(rt)) and np.array_equal(s["instance"][:, 0], ri) and np.array_equal(s["prim"][:, 0], rp)
    assert np.array_equal(bits(s["bary"][:, 0]), bits(rb))
    tpr = np.where(s["t"][:, 1] > 0, s["t"][:, 1], F(10000.0)).astype(F)   # the second hit's own t: inclusive
    rt, ri, rp, rb = instance_ref.closest(c.meshes, c.inst, c.rays, tmax_per_ray=tpr)
    s2 = mm.select(mm.all_hits_tlas(c.meshes, c.inst, c.rays, tmax_per_ray=tpr), 4)
    assert np.array_equal(bits(s2["t"][:, 0]), bits(rt)) and np.array_equal(s2["instance"][:, 0], ri)
    assert (s2["count"] <= s["count"]).all() and (s2["count"] >= np.minimum(s["count"], 2)).all()


def paged(h, k, npages, tlas):
    cur, pages = None, []
    for _ in range(npages):
        p = mm.select(h, k, after=cur)
        pages.append(p)
        cur = mm.cursor_of(p, cur, tlas)
    return pages


@pytest.mark.parametrize("k", [3, 5, 32])
def test_pages_through_the_cursor_give_the_unpaged_list(k):
    for h, tlas in ((mc.bvh_case("layers").hits, False), (mc.tlas_case().hits, True)):
        total = mm.select(h, 1)["count"]
        npages = -(-int(total.max()) // k) + 1
        whole = mm.select(h, k * npages)
        pages = paged(h, k, npages, tlas)
        for f in ("t", "instance", "prim", "bary"):
            assert np.array_equal(np.concatenate([p[f] for p in pages], axis=1), whole[f]), f
        for i, p in enumerate(pages):
            assert np.array_equal(p["count"], np.maximum(total.astype(np.int64) - k * i, 0))
        assert not pages[-1]["count"].any()


def test_order_cursor_and_padding_by_hand():
    # two coincident quads' worth of ties: triangles 0 and 1 share the diagonal, 2 and 3 repeat them 1 further along the ray
    v = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2], [-1, -1, 3], [1, -1, 3], [1, 1, 3], [-1, 1, 3]], F)
    t = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    rays = np.array([[0.5, 0.5, 0, 0, 0, 1], [0.5, -0.5, 0, 0, 0, 1], [5, 5, 0, 0, 0, 1], [0.5, 0.5, 5, 0, 0, -1]], F)
    s = mm.select(mm.all_hits(v, t, rays), 3)
    assert s["count"].tolist() == [4, 2, 0, 4]
    assert s["t"][0].tolist() == [2, 2, 3] and s["prim"][0].tolist() == [0, 1, 2]
    assert s["t"][1].tolist() == [2, 3, -1] and s["prim"][1].tolist() == [0, 2, 0xFFFFFFFF]
    assert s["t"][3].tolist() == [2, 2, 3] and s["prim"][3].tolist() == [2, 3, 0]        # from behind: nearer first, then the smaller prim
    assert (s["t"][2] == -1).all() and (s["prim"][2] == mm.NONE).all() and not s["bary"][2].any()
    assert s["bary"][0, 0].tolist() == [0.0, 0.75] and s["bary"][1, 0].tolist() == [0.5, 0.25]   # exact: every operand is a dyadic number
    # the cursor is strict in (t, prim): after (2, 0) come (2, 1) and the far quad
    s = mm.select(mm.all_hits(v, t, rays), 3, after=(np.array([2, 2, -1, 3], F), np.array([0, 0, 9, 0], np.uint32)))
    assert s["count"].tolist() == [3, 1, 0, 1]                                             # (from behind, after (3, 0): (3, 1) is left)
    assert s["t"][0].tolist() == [2, 3, 3] and s["prim"][0].tolist() == [1, 2, 3]
    # a window: the bounds are inclusive
    s = mm.select(mm.all_hits(v, t, rays, tmin=3.0, tmax=3.0), 2)
    assert s["count"].tolist() == [2, 1, 0, 2]


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------
def test_inputs_cover_ties_between_prims():
    """every tie scene: some ray has two bit-equal t on different prims; the cube's vertex rays tie more than two"""
    for name in ("cube", "layers", "floor", "blob"):
        s = mm.select(mc.bvh_case(name).hits, 32)
        assert mc.equal_t_runs(s, "prim").sum() >= 5, name
    s = mm.select(mc.bvh_case("cube").hits, 8)
    t = s["t"]
    assert ((t[:, 0] == t[:, 1]) & (t[:, 1] == t[:, 2]) & (t[:, 0] > 0)).any()


def test_inputs_cover_ties_between_instances():
    c = mc.tlas_case()
    s = mm.select(c.hits, 32)
    tie = mc.equal_t_runs(s, "instance")
    assert tie.sum() >= 100
    t, i = s["t"], s["instance"]
    same = (t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0) & (i[:, 1:] != i[:, :-1])
    assert (i[:, 1:][same] > i[:, :-1][same]).all()                       # the lower instance first
    assert 3 not in np.unique(c.hits.inst) and 4 in np.unique(c.hits.inst)   # the masked instance never, the nested one is reached


def test_inputs_cover_overflow_and_misses():
    s = mm.select(mc.bvh_case("layers").hits, 32)
    assert (s["count"] == mc.NLAYERS).sum() >= 10 and (s["count"] == 2 * mc.NLAYERS).sum() >= 10 and (s["count"] > 32).sum() >= 50
    for name in mc.BVH_CASES:
        assert (mm.select(mc.bvh_case(name).hits, 1)["count"] == 0).any(), name
    assert (mm.select(mc.tlas_case().hits, 1)["count"] == 0).any()


def test_inputs_cover_page_boundaries_inside_ties():
    """K = 5 on `layers` and K = 3 on the instances: some page ends between two hits of equal t, where only the cursor's prim / instance
    part separates the pages"""
    for h, k, field, tlas in ((mc.bvh_case("layers").hits, 5, "prim", False), (mc.tlas_case().hits, 3, "instance", True)):
        first = mm.select(h, k)
        nxt = mm.select(h, k, after=mm.cursor_of(first, None, tlas))
        split = (first["t"][:, k - 1] > 0) & (first["t"][:, k - 1] == nxt["t"][:, 0]) & (first[field][:, k - 1] != nxt[field][:, 0])
        assert split.sum() >= 5, (field, int(split.sum()))


def test_inputs_cover_the_side_list():
    """`adversarial`: more than 50 side-listed triangles, and some ray ACCEPTS one -- a hit that is also in a leaf, so it counts twice
    unless the kernels de-duplicate"""
    c = mc.bvh_case("adversarial")
    ill = mc.side_listed(c.v, c.t)
    assert ill.sum() > 50
    assert ill[c.hits.prim].sum() >= 10


# ---- the library and its Python binding ------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points(vx):
    L = vx.lib()
    for name in ("vx_bvh_trace_multi", "vx_bvh_trace_multi_device", "vx_tlas_trace_multi", "vx_tlas_trace_multi_device"):
        assert name in vx.SYMBOLS and getattr(L, name) is not None


def test_ctypes_structures_match_the_header(vx, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxhip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(vx_multihit_args), sizeof(vx_bvh_multihit_args), sizeof(vx_tlas_multihit_args), offsetof(vx_bvh_multihit_args, bary), "
                   "offsetof(vx_tlas_multihit_args, bary), offsetof(vx_tlas_multihit_args, instance), offsetof(vx_tlas_multihit_args, after_instance)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    B, T = vx.BvhMultiHitArgs, vx.TlasMultiHitArgs
    assert got == [C.sizeof(vx.MultiHitArgs), C.sizeof(B), C.sizeof(T), B.bary.offset, T.bary.offset, T.instance.offset, T.after_instance.offset]
