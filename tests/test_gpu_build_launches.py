"""GPU tests of the launches taken off a VX_GRID_VEC build's dependent chain.  (B) In a list_async rebuild the host's hit count comes from the
voxelizer's own counters, posted by the brick kernel, and the block-hit scan is queued with the list's emission -- beside the next ray batch
or on the main stream by whatever reads the list first: every order of build, rays and list.  (C) k_mip2_scan -- the level-2 mip and the
line-count scan in one launch, for one scan tile and for more.  Everything is compared whole with the CPU oracle (oracle.build_bool /
build_vec / bool_aabbs / trace_brute); which kernels ran is read from the library's launch profile."""
import numpy as np
import pytest

import oracle
import vx_scenes
from test_gpu_build_chain import box_soup, check_vec

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(1.0)


class Built:
    """the oracle's build of one mesh (what test_gpu_build_chain.check_vec compares with): computed once per mesh and left unchanged"""

    def __init__(self, v, t, dims, nrays=200, seed=3):
        self.v, self.t = v, t
        self.words, self.calls, self.gi = oracle.build_bool(v, t, VS)
        assert tuple(self.gi["dim"]) == tuple(dims), self.gi["dim"]
        self.list = oracle.build_vec(v, t, VS)
        self.boxes = oracle.bool_aabbs(self.words, self.gi, VS)
        self.rays = vx_scenes.random_rays(nrays, self.gi["bmin"], self.gi["bmax"], seed=seed)
        self.t_ref, self.prim_ref = oracle.trace_brute(self.boxes, self.rays)


def launches(gpu, fn):
    """{kernel: launches} of fn()"""
    gpu.profile_enable(True)
    gpu.profile_reset()
    try:
        fn()
        return {k: n for k, (_, n) in gpu.profile_read().items()}
    finally:
        gpu.profile_enable(False)


def scan_launches(n):
    return n.get("k_scan_onepass", 0)


# ---- (B) the hit count from the voxelizer's counters, the block-hit scan with the list ---------------------------------------------
DIMS_B = (512, 16, 16)
_b = {}


def ref_b(k):
    if k not in _b:
        _b[k] = Built(*box_soup(DIMS_B, (300, 700, 150)[k], seed=k + 1), DIMS_B, nrays=300)
    return _b[k]


def check_list(g, r, what):
    """count, list bytes and prim"""
    a = g.aabbs()
    assert len(a) == len(r.list), what + ": count"
    assert a.tobytes() == r.list.tobytes(), what + ": list"
    tt, pp, nh = g.trace(r.rays)
    assert np.array_equal(tt, r.t_ref) and np.array_equal(pp, r.prim_ref), what + ": t, prim"
    assert g.describe()["set_calls"] == r.calls == len(r.list), what + ": calls"


def test_deferred_scan_orders(gpu):
    r = [ref_b(0), ref_b(1), ref_b(2)]
    assert len({len(x.list) for x in r}) == 3
    m = [gpu.Mesh.from_arrays(x.v, x.t) for x in r]
    g = gpu.Grid.voxelize(m[1], VS, gpu.GRID_VEC)           # (the largest first: the rebuilds below fit the handle's buffers)
    check_vec(g, r[1], "first build")
    # the build queues the unit scan and the pair launch; the block-hit scan comes with the list
    n = launches(gpu, lambda: g.revoxelize(m[0], VS, list_async=True))
    assert scan_launches(n) == 1 and n.get("k_mip2_scan") == 1 and not n.get("k_emit_units"), n
    n = launches(gpu, lambda: check_list(g, r[0], "aabbs() with no trace"))
    assert scan_launches(n) == 1 and n.get("k_emit_units") == 1, n
    check_vec(g, r[0], "after the list")
    # a trace first (scan and emission beside the rays), then the list
    g.revoxelize(m[2], VS, list_async=True)
    n = launches(gpu, lambda: g.trace(r[2].rays))
    assert scan_launches(n) == 1 and n.get("k_emit_units") == 1, n
    tt, pp, _ = g.trace(r[2].rays)
    assert np.array_equal(tt, r[2].t_ref) and np.array_equal(pp, r[2].prim_ref)
    n = launches(gpu, lambda: check_list(g, r[2], "a trace first, then aabbs()"))
    assert scan_launches(n) == 0 and not n.get("k_emit_units"), n
    # two list_async rebuilds in a row with different meshes and nothing read in between (the first list and its scan are dropped)
    n = launches(gpu, lambda: (g.revoxelize(m[0], VS, list_async=True), g.revoxelize(m[1], VS, list_async=True)))
    assert scan_launches(n) == 2 and not n.get("k_emit_units"), n
    check_list(g, r[1], "two rebuilds in a row")
    check_vec(g, r[1], "two rebuilds in a row, everything")
    # list_async, then the list inside the build, and back
    g.revoxelize(m[2], VS, list_async=True)
    n = launches(gpu, lambda: g.revoxelize(m[0], VS))
    assert scan_launches(n) == 2 and n.get("k_emit_units") == 1, n      # (unit scan, and the block-hit scan in the build again)
    check_list(g, r[0], "list inside the build")
    g.revoxelize(m[2], VS, list_async=True)
    check_vec(g, r[2], "and back", rays_first=True)
    g.revoxelize(m[1], VS, list_async=True)
    check_vec(g, r[1], "and once more, the list first")


def test_deferred_scan_with_an_empty_list_and_other_grids(gpu):
    """a rebuild whose mesh sets no voxel in a grid that keeps the scan in the build (ragged rows), and one that defers it again"""
    small, ragged = ref_b(0), Built(*box_soup((70, 9, 7), 300, seed=1), (70, 9, 7), nrays=300)
    ms, mr = gpu.Mesh.from_arrays(small.v, small.t), gpu.Mesh.from_arrays(ragged.v, ragged.t)
    g = gpu.Grid.voxelize(ms, VS, gpu.GRID_VEC)
    n = launches(gpu, lambda: g.revoxelize(mr, VS, list_async=True))
    assert scan_launches(n) == 3, n            # rows that are no multiple of 32 voxels: unit scan, block-hit scan and word prefix in the build
    check_vec(g, ragged, "ragged rows", rays_first=True)
    g.revoxelize(ms, VS, list_async=True)
    check_vec(g, small, "back to rows of 512")


# ---- (C) the mip and the line-count scan in one launch -------------------------------------------------------------------------------
# 512 x 128 x 128: exactly 16 384 lines, i.e. 16 385 outputs -- a second scan tile for the total alone; the next two need two tiles of counts;
# 512 x 8 x 8: one tile and one mip word
@pytest.mark.parametrize("dims", [(512, 128, 128), (512, 128, 136), (1024, 64, 130), (512, 8, 8)], ids=lambda d: "x".join(map(str, d)))
def test_pair_launch(gpu, dims):
    r = Built(*box_soup(dims, 300, seed=1), dims, nrays=2000)   # (300 triangles in up to 8.9 M cells: 2000 rays for some dozens of hits)
    assert (r.t_ref > 0).sum() > 40
    lines = dims[0] * dims[1] * dims[2] // 32 // 16
    if dims == (512, 128, 128):
        assert lines == 16384
    assert (lines + 1 + 16383) // 16384 == (1 if dims == (512, 8, 8) else 2)
    mesh = gpu.Mesh.from_arrays(r.v, r.t)
    g = None

    def build():
        nonlocal g
        g = gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC)
    n = launches(gpu, build)
    assert n.get("k_mip2_scan") == 1 and not n.get("k_build_mip2"), n
    assert g.describe()["occupied"] == len(r.boxes)
    check_vec(g, r, "first build")
    n = launches(gpu, lambda: g.revoxelize(mesh, VS, list_async=True))
    assert n.get("k_mip2_scan") == 1 and not n.get("k_build_mip2"), n
    check_vec(g, r, "rebuild", rays_first=True)
    # a Bool handle keeps the two kernels (its list needs the word prefix)
    gb = None

    def build_bool():
        nonlocal gb
        gb = gpu.Grid.voxelize(mesh, VS, gpu.GRID_BOOL)
    n = launches(gpu, build_bool)
    assert not n.get("k_mip2_scan") and n.get("k_build_mip2") == 1, n
    assert gb.aabbs().tobytes() == r.boxes.tobytes() and gb.describe()["occupied"] == len(r.boxes)
