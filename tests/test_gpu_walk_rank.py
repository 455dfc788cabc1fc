"""GPU tests of k_walk's rank epilogue: a batch that asks for t + prim (and nothing else) on a grid with 32-bit voxel indices is ranked
by the ray kernel's own waves as they leave -- each wave ranks the rays of the chunks it drew from the work queue, which it remembers in
a ring of VOXHIP_TRACE_RING entries -- instead of by a k_rank launch behind the kernel.

Every case compares t and prim bit for bit with BOTH
  * the oracle's brute force over all occupied boxes (the definition), and
  * the same rays traced through trace_ex(want=("t", "prim", "normal")), which still goes through k_rank.
Both references are computed once per grid on a pool of rays of four kinds (hit, miss the grid box, enter the box and hit nothing,
random); a batch of any size and layout is a gather from the pool, and so is what it must return.  What a ray returns does not depend on
where in the batch it stands; where it stands decides which wave traces it, from which chunk, and that is what these cases vary.
"""
import os

import numpy as np
import pytest

import oracle
import vx_scenes

pytestmark = pytest.mark.gpu

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
POOL = 2048  # rays per kind


class env:
    """Set the library's run-time switches for the duration of a block (read at every launch); None: unset."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# name -> (cells per axis, grid flavour).  The mesh is a small lumpy sphere scaled to the box; 1/16 and the extents are exact floats, so
# the grid has exactly these cells.  Which form of the rank each grid takes (grid_mips in vx_api.cpp: the 16th-prefix table is used when
# one was written and the mask is a whole number of 16-word lines):
#   vec64:   X % 512 != 0, so the build leaves no line counts; its word-prefix scan (single pass, 8192 words) writes the 16th-prefix table
#            beside the prefix: the TABLE form, fed by the scan
#   vec512:  rows of 512 voxels, a whole Vec build: the TABLE form, fed by the brick kernel's line counts (no word prefix exists)
#   bool70, vec70:  ragged -- no axis a multiple of 8, 3610 mask words, no whole number of lines: the WORD-PREFIX form, on a Bool and on a
#            Vec build
GRIDS = {"vec64": ((64, 64, 64), "GRID_VEC"), "vec512": ((512, 16, 16), "GRID_VEC"), "bool70": ((70, 50, 33), "GRID_BOOL"),
         "vec70": ((70, 50, 33), "GRID_VEC")}
VS = F(1.0 / 16)


def _mesh_for(dim):
    v, t = vx_scenes.blob(nlon=48, nlat=47, seed=3)  # bbox exactly [-1, 1]^3
    return (v * (np.array(dim, np.float32) * VS * F(0.5))).astype(np.float32), t


def _away_rays(gi, n, seed):
    """Origins outside the grid box, directions pointing away from its centre: they cannot touch the box and retire at refill."""
    rng = np.random.default_rng(seed)
    lo, hi = gi["bmin"].astype(np.float64), gi["bmax"].astype(np.float64)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (lo + hi) / 2 + 1.5 * np.linalg.norm(hi - lo) * d
    d32 = d.astype(np.float32)
    d32[d32 == 0] = F(1e-20)
    return np.ascontiguousarray(np.concatenate([o.astype(np.float32), d32], axis=1))


class Case:
    """One grid, its pool of rays and the two references on the pool."""

    def __init__(self, gpu, name):
        dim, kind = GRIDS[name]
        v, t = _mesh_for(dim)
        self.mesh = gpu.Mesh.from_arrays(v, t)
        self.kind = getattr(gpu, kind)
        self.g = gpu.Grid.voxelize(self.mesh, VS, self.kind)
        ow, _, gi = oracle.build_bool(v, t, VS)
        assert gi["dim"] == dim and self.g.describe()["dim"] == dim and np.array_equal(self.g.bitmask(), ow)
        self.v, self.t, self.gi = v, t, gi
        oa = oracle.bool_aabbs(ow, gi, VS)
        # candidates: random rays aimed into the box (most hit the blob, those through the box's corners do not)
        cand = vx_scenes.random_rays(16 * POOL, gi["bmin"], gi["bmax"], seed=11)
        ct, _ = oracle.trace_brute(oa, cand)
        hit, thru = cand[ct > 0][:POOL], cand[ct < 0][:POOL]
        assert len(hit) == POOL and len(thru) >= POOL // 8, (len(hit), len(thru))
        thru = thru[np.arange(POOL) % len(thru)]
        away = _away_rays(gi, POOL, 12)
        rnd = vx_scenes.random_rays(POOL, gi["bmin"], gi["bmax"], seed=13)
        self.pool = np.ascontiguousarray(np.concatenate([hit, away, thru, rnd]))
        self.kinds = dict(hit=0, away=1, thru=2, rnd=3)
        self.ref_t, self.ref_p = oracle.trace_brute(oa, self.pool)
        assert np.all(self.ref_t[:POOL] > 0) and np.all(self.ref_t[POOL:3 * POOL] < 0) and np.all(self.ref_p[POOL:3 * POOL] == MISS)
        k = self.g.trace_ex(self.pool, want=("t", "prim", "normal"))  # the k_rank path
        assert np.array_equal(k["t"], self.ref_t) and np.array_equal(k["prim"], self.ref_p)

    def sel(self, kind, n, seed=0):
        """n pool indices of one kind, in a shuffled order"""
        rng = np.random.default_rng(seed + n)
        return (self.kinds[kind] * POOL + rng.integers(0, POOL, n)).astype(np.int64)

    def mix(self, name, n):
        if name == "interleaved":  # hit, miss, hit, miss ...
            idx = self.sel("hit", n)
            idx[1::2] = self.sel("away", n)[1::2]
            return idx
        return self.sel({"hits": "hit", "misses": "away", "through": "thru"}[name], n)

    def check(self, idx, what):
        """trace pool[idx] through the t + prim query and compare with the references"""
        tt, pp, nh = self.g.trace(self.pool[idx])
        assert np.array_equal(tt, self.ref_t[idx]), what
        assert np.array_equal(pp, self.ref_p[idx]), what
        assert nh == int((self.ref_t[idx] > 0).sum()), what


@pytest.fixture(scope="module")
def cases(gpu):
    """the grids with their pools and references, built on first use, freed when the module is done"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(gpu, name)
        return made[name]

    yield get
    for c in made.values():
        c.g.free()
        c.mesh = None


@pytest.fixture(params=list(GRIDS))
def case(cases, request):
    return cases(request.param)


# 1 .. 4097: one workgroup and less than a wave up to a few workgroups; 100 000: static chunks only (n <= 64 rays x waves); 300 001: dynamic
# chunks, the last one clipped; 399 999 / 400 000: either side of the n / 1040 workgroup rule
SIZES = (1, 63, 64, 65, 4097, 100_000, 300_001, 399_999, 400_000)
MIXES = ("hits", "misses", "interleaved", "through")


def test_batch_sizes_and_ray_mixes(case):
    for n in SIZES:
        for m in MIXES:
            case.check(case.mix(m, n), (n, m))


@pytest.mark.parametrize("lds,donate", [(0, None), (None, 0), (0, 0)])
def test_forced_kernel_variants(case, lds, donate):
    """global-memory mips (VOXHIP_TRACE_LDS=0) and no work donation (VOXHIP_TRACE_DONATE=0); the default pair is every other test"""
    with env(VOXHIP_TRACE_LDS=lds, VOXHIP_TRACE_DONATE=donate):
        for n in SIZES:
            case.check(case.mix("interleaved", n), (n, lds, donate))
        for m in MIXES:
            case.check(case.mix(m, 300_001), (m, lds, donate))


@pytest.mark.parametrize("ring", [1, 2])
def test_full_ring(case, ring):
    """300 001 rays are 4096 waves with static chunks of 64 rays and 592 dynamic chunks.  The rays of the first 64 waves' static chunks and
    all rays behind the static part miss the box, the ones in between hit: the 64 idle waves race through the dynamic chunks and fill
    rings of one or two entries, after which they must leave the rest to the others.  (Whether a ring filled cannot be observed; the
    results must be right either way.)"""
    n = 300_001
    idx = case.sel("hit", n)
    away = case.sel("away", n, seed=1)
    idx[:64 * 64] = away[:64 * 64]
    idx[4096 * 64:] = away[4096 * 64:]
    with env(VOXHIP_TRACE_RING=ring):
        case.check(idx, ring)
        case.check(case.mix("interleaved", 400_000), ring)
    with env(VOXHIP_TRACE_RING=0):  # the switch's other end: k_rank
        case.check(idx, 0)


def test_back_to_back_batches_on_one_handle(case):
    """different n, no synchronisation in between: the two work counters alternate and the ring is reused"""
    import torch
    ns = (300_001, 4097, 399_999, 65, 400_000)
    idxs = [case.mix("interleaved" if k & 1 else "hits", n) for k, n in enumerate(ns)]
    d_rays = [torch.from_numpy(case.pool[i]).cuda() for i in idxs]
    d_t = [torch.zeros(n, dtype=torch.float32, device="cuda") for n in ns]
    d_p = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in ns]
    torch.cuda.synchronize()
    for r, n, a, b in zip(d_rays, ns, d_t, d_p):
        case.g.trace_device(r.data_ptr(), n, a.data_ptr(), b.data_ptr())
    torch.cuda.synchronize()
    for i, a, b in zip(idxs, d_t, d_p):
        assert np.array_equal(a.cpu().numpy(), case.ref_t[i]) and np.array_equal(b.cpu().numpy().view(np.uint32), case.ref_p[i]), len(i)


def test_no_prim_wanted(case):
    """prim_ptr=None: no epilogue, and nothing is written where an earlier batch's prim went"""
    import torch
    n = 300_001
    idx = case.mix("interleaved", n)
    d_rays = torch.from_numpy(case.pool[idx]).cuda()
    d_t = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_p = torch.zeros(n, dtype=torch.int32, device="cuda")
    case.g.trace_device(d_rays.data_ptr(), n, d_t.data_ptr(), d_p.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_p.cpu().numpy().view(np.uint32), case.ref_p[idx])
    d_p.fill_(0x5A5A5A5A)
    d_t.zero_()
    torch.cuda.synchronize()
    case.g.trace_device(d_rays.data_ptr(), n, d_t.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy(), case.ref_t[idx])
    assert bool((d_p == 0x5A5A5A5A).all())


def test_primary_camera(case, gpu):
    """trace_primary_device on a 96 x 64 camera: in-kernel rays.  Bit-equal to the k_rank path on the same camera; against the brute force
    on the oracle's explicit rays as tests/test_gpu_configs.py compares in-kernel rays: they differ from the explicit ones by the rounding
    of the normalisation only, so prim agrees on more than 98 % of the pixels and t, where prim agrees, within 1e-5."""
    import torch
    W, H = 96, 64
    gi = case.gi
    ctr = (gi["bmin"] + gi["bmax"]).astype(np.float64) / 2
    ext = float(np.linalg.norm(gi["bmax"] - gi["bmin"]))
    vi, pi = vx_scenes.camera_matrices(eye=tuple(ctr + np.array([0.35, 0.25, 0.9]) * ext), ctr=tuple(ctr), fov_deg=50.0, aspect=W / H)
    d_t = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    d_p = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    case.g.trace_primary_device(vi, pi, W, H, d_t.data_ptr(), d_p.data_ptr())
    torch.cuda.synchronize()
    tt, pp = d_t.cpu().numpy(), d_p.cpu().numpy().view(np.uint32)
    k = case.g.trace_ex(camera=(vi, pi, W, H), want=("t", "prim", "normal"))
    assert np.array_equal(tt, k["t"]) and np.array_equal(pp, k["prim"])
    ow = case.g.bitmask()
    ot, op = oracle.trace_brute(oracle.bool_aabbs(ow, gi, VS), oracle.primary_rays(vi, pi, W, H))
    same = pp == op
    assert same.mean() > 0.98 and np.allclose(tt[same], ot[same], rtol=0, atol=1e-5)
    assert (ot > 0).sum() > 50  # (the 512 x 16 x 16 grid is a thin bar in this view)


def test_trace_after_stream_change(gpu):
    """a rebuild that moves the handle to another stream, then a batch: the ring, like every buffer of the handle, follows the stream"""
    import torch
    c = Case(gpu, "vec64")
    idx = c.mix("interleaved", 300_001)
    c.check(idx, "default stream")
    s = torch.cuda.Stream()
    c.g.revoxelize(c.mesh, VS, stream=s.cuda_stream)
    c.check(idx, "side stream")
    c.check(c.mix("hits", 4097), "side stream, smaller batch")
    s.synchronize()
    c.g.free()


@pytest.mark.parametrize("name", ["vec64", "vec512"])
def test_list_async_rebuild_then_batch(gpu, name):
    """A Vec rebuild whose list is emitted beside the next ray batch (side stream, behind the gate on the ray kernel's work counter): the
    batch is ranked in the kernel, and the list is the oracle's, byte for byte."""
    c = Case(gpu, name)
    ov = oracle.build_vec(c.v, c.t, VS)
    for n in (300_001, 100_000):  # with dynamic chunks, and static chunks only (the counter is never touched: the gate's time bound)
        c.g.revoxelize(c.mesh, VS, list_async=True)
        c.check(c.mix("interleaved", n), n)
        assert c.g.aabbs().tobytes() == ov.tobytes()
    c.g.free()
