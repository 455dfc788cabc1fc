"""GPU tests of the Vec build's shortened chain.  (1) On grids whose rows are multiples of 512 voxels the brick kernel leaves the set bits of every
16-word line of the bitmask, their scan is the rank pass's table of every 16th word prefix (and its total the occupied count), and the
word prefix itself is built only for whoever indexes it -- the Bool list, materials, surface materials, multi-hit.  Every result is
compared whole with the CPU oracle (oracle.build_bool / build_vec / bool_aabbs / trace_brute) or with the restatements the neighbouring
test files use; grids that keep the word-prefix scan (rows that are no multiple of 512, nwords % 16 != 0, ragged rows) run beside them.
(2) A VX_VOXELIZE_LIST_ASYNC rebuild queues the voxelizer before the host knows the unit total, sized by the previous build's buffers: rebuilds
with many more and many fewer units, after a failed build, and the status codes."""
import numpy as np
import pytest

import multihit_ref as mr
import oracle
import vx_scenes
from test_gpu_components import check as check_components
from test_gpu_multihit import same as same_hits
from test_gpu_parity import _material_scene, _value_ids
from test_gpu_surface import check_surface

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(1.0)


def box_soup(dims, ntri=300, seed=1, edge=3.0):
    """Small random triangles inside [0, X] x [0, Y] x [0, Z]; two vertices pin the bounding box, so at voxel size 1 the grid has exactly
    `dims` cells."""
    rng = np.random.default_rng(seed)
    d = np.asarray(dims, np.float64)
    p = rng.uniform(0, 1, (ntri, 1, 3)) * d + rng.uniform(-edge, edge, (ntri, 3, 3))
    p = np.clip(p, 0, d)
    p[0, 0] = 0
    p[1, 0] = d
    return p.reshape(-1, 3).astype(np.float32), np.arange(3 * ntri, dtype=np.int32).reshape(-1, 3)


class Ref:
    """the oracle's build of one mesh: computed once per mesh and left unchanged"""

    def __init__(self, dims, ntri=300, seed=1):
        self.v, self.t = box_soup(dims, ntri, seed)
        self.words, self.calls, self.gi = oracle.build_bool(self.v, self.t, VS)
        assert tuple(self.gi["dim"]) == tuple(dims)
        self.list = oracle.build_vec(self.v, self.t, VS)
        self.boxes = oracle.bool_aabbs(self.words, self.gi, VS)
        self.rays = vx_scenes.random_rays(300, self.gi["bmin"], self.gi["bmax"], seed=seed + 5)
        self.t_ref, self.prim_ref = oracle.trace_brute(self.boxes, self.rays)
        assert (self.t_ref > 0).sum() > 20


_refs = {}


def ref_of(dims, ntri=300, seed=1):
    key = (tuple(dims), ntri, seed)
    if key not in _refs:
        _refs[key] = Ref(dims, ntri, seed)
    return _refs[key]


def check_vec(g, r, what="", rays_first=False):
    """mask, list, counts and the first hits (t and prim) of a Vec handle against the oracle's (rays_first: the ray batch is the first thing
    queued behind the build, so a deferred list is written beside it)"""
    if rays_first:
        tt, pp, _ = g.trace(r.rays)
        assert np.array_equal(tt, r.t_ref) and np.array_equal(pp, r.prim_ref), what + ": first batch"
    assert np.array_equal(g.bitmask(), r.words), what + ": bitmask"
    a = g.aabbs()
    assert len(a) == len(r.list) and a.tobytes() == r.list.tobytes(), what + ": Vec list"
    tt, pp, nh = g.trace(r.rays)
    assert np.array_equal(tt, r.t_ref), what + ": t"
    assert np.array_equal(pp, r.prim_ref), what + ": prim"
    assert nh == int((r.t_ref > 0).sum())
    d = g.describe()
    assert d["occupied"] == len(r.boxes) and d["set_calls"] == r.calls, what + ": counts"


# rows of 512 k voxels take the line counts (one, two and three 512-voxel chunks per row; one brick row and several; more than one scan
# tile of counts would need 2^18 lines and is the bench's own case); the others keep the word-prefix scan: whole words with nwords % 16 == 0
# and != 0, ragged rows
GRIDS = [(32, 32, 32), (64, 32, 32), (512, 8, 8), (96, 8, 5), (70, 9, 7), (512, 24, 40), (1024, 4, 4), (1536, 3, 5), (512, 9, 7)]


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_prim_ranks(gpu, dims):
    r = ref_of(dims)
    nwords = (dims[0] * dims[1] * dims[2] + 31) // 32
    if dims == (32, 32, 32):
        assert nwords // 16 == 64
    if dims == (96, 8, 5):
        assert nwords % 16 != 0
    g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(r.v, r.t), VS, gpu.GRID_VEC)
    check_vec(g, r, "x".join(map(str, dims)))
    # the ranks again once the word prefix exists beside the table (multi-hit builds it), and the occupied count
    k = 3
    ref = mr.select(mr.hit_times(r.boxes, r.rays.astype(np.float32)), k)
    same_hits(g.trace_multi(r.rays, max_hits=k), ref, "multi-hit")
    tt, pp, _ = g.trace(r.rays)
    assert np.array_equal(tt, r.t_ref) and np.array_equal(pp, r.prim_ref)


def consumers(gpu, g, r, mesh):
    """everything that indexes the word prefix itself, on a Vec handle built without it"""
    k = 4
    ref = mr.select(mr.hit_times(r.boxes, r.rays.astype(np.float32)), k)
    same_hits(g.trace_multi(r.rays, max_hits=k), ref, "multi-hit")
    check_surface(g, device=False)
    check_components(g, connectivity=(6,), device=False)
    # the Bool list of a Bool handle of the same mesh
    gb = gpu.Grid.voxelize(mesh, VS, gpu.GRID_BOOL)
    assert gb.aabbs().tobytes() == r.boxes.tobytes()
    assert gb.describe()["occupied"] == len(r.boxes)
    tt, pp, _ = gb.trace(r.rays)
    assert np.array_equal(tt, r.t_ref) and np.array_equal(pp, r.prim_ref)
    # ... and the ranks of the Vec handle after all of them
    tt, pp, _ = g.trace(r.rays)
    assert np.array_equal(tt, r.t_ref) and np.array_equal(pp, r.prim_ref)


def test_lazy_word_prefix_consumers_and_rebuild(gpu):
    """A Vec build, then each consumer of the full word prefix; the same after a rebuild of the handle with another mesh (a prefix of the
    first mask must not survive), in both orders of table and prefix."""
    dims = (512, 16, 16)
    r1, r2 = ref_of(dims, 300, 1), ref_of(dims, 500, 2)
    m1, m2 = gpu.Mesh.from_arrays(r1.v, r1.t), gpu.Mesh.from_arrays(r2.v, r2.t)
    g = gpu.Grid.voxelize(m1, VS, gpu.GRID_VEC)
    consumers(gpu, g, r1, m1)
    check_vec(g, r1, "first build")
    g.revoxelize(m2, VS)
    consumers(gpu, g, r2, m2)          # the word prefix first, then the ranks
    check_vec(g, r2, "second build")
    g.revoxelize(m1, VS)
    check_vec(g, r1, "third build")    # the ranks first ...
    consumers(gpu, g, r1, m1)          # ... then the word prefix


def test_materials_between_plain_builds(gpu):
    """A materials build indexes the word prefix inside the build: on a handle whose previous build left only the table, and back."""
    dims = (512, 16, 16)
    r = ref_of(dims, 300, 1)
    rng = np.random.default_rng(3)
    nmat = 4
    recs = _material_scene("cube", nmat, 1)[2]
    ids = rng.integers(-1, nmat, len(r.t)).astype(np.int32)
    tv, nvalues, _ = _value_ids(recs, ids)
    mesh = gpu.Mesh.from_arrays(r.v, r.t)
    mesh.set_materials(recs, ids)
    g = gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC)
    check_vec(g, r, "plain")
    g.revoxelize(mesh, VS, materials=True)
    mats, mid = g.materials()
    oids, order = oracle.material_ids(r.v, r.t, VS, tv, nvalues, per_call=True, ncalls=r.calls)
    assert np.array_equal(mid, oids) and len(mats) == len(order)
    check_vec(g, r, "materials")
    gb = gpu.Grid.voxelize(mesh, VS, gpu.GRID_BOOL, materials=True)
    oidb, _ = oracle.material_ids(r.v, r.t, VS, tv, nvalues, per_call=False, ncalls=r.calls)
    assert np.array_equal(gb.materials()[1], oidb)
    g.revoxelize(mesh, VS)
    check_vec(g, r, "plain again")
    check_surface(g, materials=False, device=False)


def test_rebuilds_across_paths_and_sizes(gpu):
    """One handle rebuilt with grids that take the line counts and grids that keep the word-prefix scan, larger and smaller, with and
    without the list beside the rays: the table, the count and the list belong to the last build every time."""
    seq = [((512, 8, 8), 1), ((70, 9, 7), 1), ((1024, 4, 4), 1), ((512, 24, 40), 1), ((96, 8, 5), 1), ((512, 8, 8), 1), ((32, 32, 32), 1), ((512, 16, 16), 2)]
    g = None
    for k, (dims, seed) in enumerate(seq):
        r = ref_of(dims, 500 if seed == 2 else 300, seed)
        mesh = gpu.Mesh.from_arrays(r.v, r.t)
        if g is None:
            g = gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC)
        else:
            g.revoxelize(mesh, VS, list_async=bool(k & 1))
        if k % 3 == 2:   # the count before anything else asks for the table
            assert g.describe()["occupied"] == len(r.boxes)
        check_vec(g, r, "build %d" % k)


def test_two_handles_on_two_streams(gpu):
    """Two Vec handles rebuilt and traced alternately on streams of their own, twice in a row each."""
    import torch
    dims = (512, 16, 16)
    refs = [ref_of(dims, 300, 1), ref_of(dims, 500, 2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    meshes = [gpu.Mesh.from_arrays(r.v, r.t) for r in refs]
    grids = [gpu.Grid.voxelize(meshes[k], VS, gpu.GRID_VEC, stream=streams[k].cuda_stream) for k in range(2)]
    d_rays = [torch.from_numpy(np.ascontiguousarray(r.rays, np.float32)).cuda() for r in refs]
    d_t = [torch.empty(len(r.rays), dtype=torch.float32, device="cuda") for r in refs]
    d_p = [torch.empty(len(r.rays), dtype=torch.int32, device="cuda") for r in refs]
    torch.cuda.synchronize()
    for rnd in range(2):
        for k in range(2):
            w = (k + rnd) % 2   # the handles swap meshes every round
            grids[k].revoxelize(meshes[w], VS, stream=streams[k].cuda_stream)
            grids[k].trace_device(d_rays[w].data_ptr(), len(refs[w].rays), d_t[k].data_ptr(), d_p[k].data_ptr())
        torch.cuda.synchronize()
        for k in range(2):
            w = (k + rnd) % 2
            assert np.array_equal(d_t[k].cpu().numpy(), refs[w].t_ref)
            assert np.array_equal(d_p[k].cpu().numpy().view(np.uint32), refs[w].prim_ref)
            check_vec(grids[k], refs[w], "round %d handle %d" % (rnd, k))


def test_voxelizer_queued_ahead_of_the_unit_total(gpu):
    """list_async rebuilds of one handle: about ten times the units of the previous build (its buffers are too small: the build runs again
    with the total known), about a tenth (the hit scan runs over the zeroed tail), the same again, and after a build that failed."""
    small, big = ref_of((512, 8, 8), 60, 3), ref_of((512, 24, 40), 900, 4)
    assert len(big.list) > 8 * len(small.list)
    ms, mb = gpu.Mesh.from_arrays(small.v, small.t), gpu.Mesh.from_arrays(big.v, big.t)
    g = gpu.Grid.voxelize(ms, VS, gpu.GRID_VEC)
    check_vec(g, small, "first build")
    for k, (m, r, what) in enumerate([(mb, big, "ten times the units"), (mb, big, "the same again"), (ms, small, "a tenth of the units"),
                                      (ms, small, "small again"), (mb, big, "big after small, buffers still large")]):
        gpu.profile_enable(True)
        gpu.profile_reset()
        try:
            g.revoxelize(m, VS, list_async=True)
            n = gpu.profile_read()["k_voxelize"][1]
        finally:
            gpu.profile_enable(False)
        assert n == (2 if k == 0 else 1), what   # only the build that outgrew the buffers runs its voxelizer again
        check_vec(g, r, what, rays_first=bool(k & 1))
    # a build that fails after it queued work: more than 2^21 cells on an axis -> VX_ERR_CAPACITY, the handle is left empty
    for la in (True, False):
        with pytest.raises(gpu.VxError) as ei:
            g.revoxelize(mb, F(1e-4), list_async=la)
        assert ei.value.status == 8
        d = g.describe()
        assert tuple(d["dim"]) == (0, 0, 0) and d["occupied"] == 0 and len(g.aabbs()) == 0
        g.revoxelize(ms, VS, list_async=True)
        check_vec(g, small, "after the failed build", rays_first=la)
    # an empty mesh range and a mesh without triangles keep the first build's way
    g.revoxelize(mb, VS, list_async=True, tris=(5, 5))
    assert g.describe()["occupied"] == 0 and len(g.aabbs()) == 0
    g.revoxelize(mb, VS, list_async=True)
    check_vec(g, big, "after the empty build", rays_first=True)
