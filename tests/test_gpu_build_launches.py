"""GPU tests of the launches taken off a VX_GRID_VEC build's dependent chain.  (B) In a list_async rebuild the host's hit count comes from the
voxelizer's own counters, posted by the brick kernel, and the block-hit scan is queued with the list's emission -- beside the next ray batch
or on the main stream by whatever reads the list first: every order of build, rays and list.  (C) k_mip2_scan -- the level-2 mip and the
line-count scan in one launch, for one scan tile and for more.  Everything is compared whole with the CPU oracle (oracle.build_bool /
build_vec / bool_aabbs / trace_brute); which kernels ran is read from the library's launch profile.  (D) Every path of the build with the
kernels it launches written down as a table, and the same builds in a shuffled order on one handle per flavour."""
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


# ---- (D) which kernels each build path launches --------------------------------------------------------------------------------------
# Every path of the build -- first builds and rebuilds of the three flavours on a grid per mask form, the list beside the rays, the early
# launch and its retry, materials, solid, word shards on either side of the size rule, a word range, empty builds, a rebuild after a
# failed one -- with the kernels it launches written down: for the build call, for the first trace() behind it (where a deferred list is
# emitted beside the rays) and for aabbs() after that (list_resolve).  EXPECTED at the end of the file was recorded from a run of these
# cases (launch_table below) on commit 5c17f50, before the build was split into phases; a change of the build's host code must leave it as
# it is.  Memsets do not pass the profile, so the same builds run once more on ONE handle per flavour in a shuffled order: a stale bit of
# a larger, smaller, tiled or untiled predecessor shows in the mask, the counts or the list.
import solid_ref
from test_gpu_parity import _material_scene, _value_ids

G_LINES, G_PREFIX, G_ODD, G_RAGGED = (512, 8, 8), (64, 32, 32), (96, 8, 5), (70, 9, 7)
SMALL, BIG = ((512, 8, 8), 60, 3), ((512, 24, 40), 900, 4)      # test_gpu_build_chain's pair: the second outgrows the first one's buffers
FEW = (G_LINES, 12, 1)                                           # below the shard_small rule (MANY = soup(G_LINES) is above it)
KIND_NAMES = ("bool", "aabbstruct", "vec")


def soup(dims):
    return (dims, 300, 1)


def op(mesh, **kw):
    """one build call: the mesh (dims, triangles, seed) and revoxelize's keywords; fail: at a voxel size whose grid exceeds 2^21 cells on an
    axis (VX_ERR_CAPACITY after work was queued); no_tris: the vertices alone"""
    return dict(mesh=mesh, **kw)


def _cases():
    out = []
    for dims in (G_LINES, G_PREFIX, G_ODD, G_RAGGED):
        tag = "x".join(map(str, dims))
        for kind in KIND_NAMES:
            out.append((tag + "-" + kind + "-first", kind, [], op(soup(dims))))
            out.append((tag + "-" + kind + "-rebuild", kind, [op(soup(dims))], op(soup(dims))))
        out.append((tag + "-vec-async-fits", "vec", [op(soup(dims))], op(soup(dims), list_async=True)))
    out.append(("vec-async-outgrows", "vec", [op(SMALL)], op(BIG, list_async=True)))
    for kind in ("bool", "vec"):
        out.append((kind + "-materials", kind, [], op(soup(G_LINES), materials=True)))
        out.append((kind + "-solid", kind, [], op(soup(G_PREFIX), solid=True)))
        out.append((kind + "-shard-tiled", kind, [], op(soup(G_LINES), shard=(0, 2))))
        out.append((kind + "-shard-direct", kind, [], op(FEW, shard=(0, 2))))
        out.append((kind + "-no-triangles", kind, [], op(soup(G_LINES), no_tris=True)))
    out.append(("bool-words", "bool", [], op(soup(G_PREFIX), words=(512, 1100))))
    out.append(("vec-empty-range", "vec", [op(soup(G_LINES))], op(soup(G_LINES), tris=(5, 5), list_async=True)))
    out.append(("bool-empty-range", "bool", [], op(soup(G_LINES), tris=(5, 5))))
    out.append(("vec-after-failed", "vec", [op(SMALL), op(BIG, fail=True, list_async=True)], op(SMALL, list_async=True)))
    out.append(("bool-after-failed", "bool", [op(soup(G_LINES)), op(soup(G_LINES), fail=True)], op(soup(G_LINES))))
    return out


CASES = _cases()
_built, _views, _meshes = {}, {}, {}


def built_of(key):
    if key not in _built:
        dims, ntri, seed = key
        _built[key] = Built(*box_soup(dims, ntri, seed=seed), dims, nrays=300, seed=seed + 5)
    return _built[key]


def tiled_mask_words(dims):
    """launch_voxelize's tiled build mask: 4 x 4 rows of 32 cells per 16-word tile"""
    return (dims[2] + 3) // 4 * ((dims[1] + 3) // 4) * (dims[0] // 32) * 16


class View:
    """what the oracle says one build call leaves: the mask, the list (Vec: one record per setVoxel call; else the mask's boxes), the
    counts and the first hits.  A word shard or range keeps the calls that land in its words; an empty range or mesh keeps nothing."""

    def __init__(self, gpu, o):
        r = built_of(o["mesh"])
        dims = o["mesh"][0]
        self.rays, self.dims = r.rays, dims
        nw = len(r.words)
        self.words = np.zeros_like(r.words)
        self.interior = 0
        if o.get("no_tris") or o.get("tris"):
            self.calls = r.list[:0]
        else:
            wb, we = 0, nw
            if o.get("shard"):
                wb, we, _ = gpu.shard_words(nw, *o["shard"])
            if o.get("words"):
                wb, we = o["words"]
            self.words[wb:we] = r.words[wb:we]
            h = oracle.hits(r.v, r.t, VS).astype(np.uint64)
            assert len(h) == len(r.list) == r.calls
            word = (h[:, 0] + dims[0] * (h[:, 1] + dims[1] * h[:, 2])) // 32
            self.calls = r.list[(word >= wb) & (word < we)]
            if o.get("solid"):
                self.words, hw, self.interior = solid_ref.fill(r.words, dims)
                self.calls = solid_ref.solid_vec(r.list, hw, r.gi, VS)
        self.occupied = int(np.unpackbits(self.words.view(np.uint8)).sum())
        self.boxes = oracle.bool_aabbs(self.words, r.gi, VS)
        self.t_ref, self.prim_ref = oracle.trace_brute(self.boxes, self.rays) if len(self.boxes) else (None, None)


def view_of(gpu, o):
    key = repr(sorted((k, v) for k, v in o.items() if k not in ("list_async", "materials", "fail")))
    if key not in _views:
        _views[key] = View(gpu, o)
    return _views[key]


def _materials_of(r):
    rng = np.random.default_rng(3)
    recs = _material_scene("cube", 4, 1)[2]
    return recs, rng.integers(-1, 4, len(r.t)).astype(np.int32)


def mesh_of(gpu, o):
    key = (o["mesh"], bool(o.get("no_tris")), bool(o.get("materials")))
    if key not in _meshes:
        r = built_of(o["mesh"])
        m = gpu.Mesh.from_arrays(r.v, r.t[:0] if o.get("no_tris") else r.t)
        if o.get("materials"):
            m.set_materials(*_materials_of(r))
        _meshes[key] = m
    return _meshes[key]


def apply(gpu, g, kind, o):
    """the build call of `o` on handle g (None: a first build) -> the handle"""
    kw = {k: o[k] for k in ("list_async", "materials", "solid", "shard", "words", "tris") if k in o}
    mesh = mesh_of(gpu, o)
    if o.get("fail"):
        with pytest.raises(gpu.VxError) as ei:
            g.revoxelize(mesh, F(1e-4), **kw)
        assert ei.value.status == 8
        return g
    if g is None:
        assert "list_async" not in kw
        return gpu.Grid.voxelize(mesh, VS, getattr(gpu, "GRID_" + kind.upper()), **kw)
    g.revoxelize(mesh, VS, **kw)
    return g


def verify(gpu, g, kind, o, what, traced=None, listed=None):
    """mask, counts, list and first hits of handle g after the build call `o`, against the oracle (traced / listed: the results of the
    trace() and aabbs() calls the caller has made already)"""
    if o.get("fail"):
        d = g.describe()
        assert tuple(d["dim"]) == (0, 0, 0) and d["occupied"] == 0 and d["set_calls"] == 0 and len(g.aabbs()) == 0, what
        return
    e = view_of(gpu, o)
    tt, pp, nh = traced if traced is not None else g.trace(e.rays)
    a = listed if listed is not None else g.aabbs()
    d = g.describe()
    assert tuple(d["dim"]) == tuple(e.dims), what + ": dims"
    assert np.array_equal(g.bitmask(), e.words), what + ": bitmask"
    assert d["occupied"] == e.occupied, what + ": occupied"
    assert d["set_calls"] == len(e.calls), what + ": set_calls"
    exp = e.calls if kind == "vec" else e.boxes
    assert len(a) == len(exp) and a.tobytes() == exp.tobytes(), what + ": list"
    if e.t_ref is None:
        assert nh == 0, what + ": hits on an empty grid"
    else:
        assert np.array_equal(tt, e.t_ref) and np.array_equal(pp, e.prim_ref) and nh == int((e.t_ref > 0).sum()), what + ": t, prim"
    if o.get("solid"):
        assert g.interior() == e.interior, what + ": interior"
    if o.get("materials") and len(e.calls):
        r = built_of(o["mesh"])
        recs, ids = _materials_of(r)
        tv, nvalues, _ = _value_ids(recs, ids)
        oids, order = oracle.material_ids(r.v, r.t, VS, tv, nvalues, per_call=kind == "vec", ncalls=r.calls)
        mats, mid = g.materials()
        assert np.array_equal(mid, oids) and len(mats) == len(order), what + ": material ids"


def measure(gpu, case):
    """-> handle, [launches of the build call, of the first trace, of aabbs()], the trace's and the list's results"""
    name, kind, prep, o = case
    g = None
    for p in prep:
        g = apply(gpu, g, kind, p)
    box = {}
    n = [launches(gpu, lambda: box.update(g=apply(gpu, g, kind, o)))]
    g = box["g"]
    n.append(launches(gpu, lambda: box.update(t=g.trace(view_of(gpu, o).rays))))
    n.append(launches(gpu, lambda: box.update(a=g.aabbs())))
    return g, [{k: c for k, c in x.items() if c} for x in n], box["t"], box["a"]


def launch_table(gpu):
    """{case: [build, trace, aabbs]}: what EXPECTED was recorded with"""
    return {c[0]: measure(gpu, c)[1] for c in CASES}


def test_shard_cases_lie_on_either_side_of_the_size_rule():
    """a word shard goes through the tiled build mask when the mask is small against the mesh: tiled_mask_words * 4 / 256 <= triangles"""
    limit = tiled_mask_words(G_LINES) * 4 // 256
    assert FEW[1] < limit <= soup(G_LINES)[1] and G_LINES[0] % 32 == 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_build_path_launches(gpu, case):
    name, kind, prep, o = case
    g, n, traced, listed = measure(gpu, case)
    print(name, n)
    assert n == EXPECTED[name], name
    if name == "vec-async-outgrows":
        assert n[0]["k_voxelize"] == 2
    verify(gpu, g, kind, o, name, traced, listed)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_build_paths_on_one_handle_in_shuffled_order(gpu, kind):
    ops, seen = [], set()
    for c in CASES:
        for o in c[2] + [c[3]]:
            # (a Vec list is sharded by triangle range; under a word range that cuts a z slab the header defines the mask alone)
            if repr(sorted(o.items())) not in seen and not (kind == "vec" and "words" in o):
                seen.add(repr(sorted(o.items())))
                ops.append(o)
    order = np.random.default_rng(20).permutation(len(ops))
    g = apply(gpu, None, kind, op(soup(G_RAGGED)))
    for k, i in enumerate(order):
        g = apply(gpu, g, kind, ops[i])
        verify(gpu, g, kind, ops[i], "build %d: %r" % (k, ops[i]))


def _row(s):
    """"bbox scan_onepass:2" -> {"k_bbox": 1, "k_scan_onepass": 2}"""
    return {"k_" + w.split(":")[0]: int((w + ":1").split(":")[1]) for w in s.split()}


# case: the build call, the first trace() after it, aabbs() after that (kernel names without their k_, launches behind a colon when not 1)
EXPECTED = {name: [_row(s) for s in rows] for name, rows in {
    "512x8x8-bool-first": ("bbox build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "512x8x8-bool-rebuild": ("bbox build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "512x8x8-aabbstruct-first": ("bbox build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "512x8x8-aabbstruct-rebuild": ("bbox build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "512x8x8-vec-first": ("bbox build_bricks3 emit_units mip2_scan scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", ""),
    "512x8x8-vec-rebuild": ("bbox build_bricks3 emit_units mip2_scan scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", ""),
    "512x8x8-vec-async-fits": ("bbox build_bricks3 mip2_scan scan_onepass tri_setup unit_blocks voxelize",
        "emit_units scan_onepass walk", ""),
    "64x32x32-bool-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "64x32x32-bool-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "64x32x32-aabbstruct-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "64x32x32-aabbstruct-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "64x32x32-vec-first": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "64x32x32-vec-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "64x32x32-vec-async-fits": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "emit_units scan_onepass walk", ""),
    "96x8x5-bool-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "96x8x5-bool-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "96x8x5-aabbstruct-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "96x8x5-aabbstruct-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "96x8x5-vec-first": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "96x8x5-vec-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "96x8x5-vec-async-fits": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "emit_units scan_onepass walk", ""),
    "70x9x7-bool-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "70x9x7-bool-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "70x9x7-aabbstruct-first": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "70x9x7-aabbstruct-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "70x9x7-vec-first": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "70x9x7-vec-rebuild": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "70x9x7-vec-async-fits": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:3 tri_setup unit_blocks voxelize",
        "emit_units walk", ""),
    "vec-async-outgrows": ("bbox:2 build_bricks3:2 mip2_scan:2 scan_onepass:3 tri_setup:2 unit_blocks:2 voxelize:2",
        "emit_units walk", ""),
    "bool-materials": ("bbox build_bricks3 build_mip2 mat_ids mat_last scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
    "bool-solid": ("bbox brick_mip1 build_bricks3 build_mip2 scan_onepass:3 solid_col:8 solid_col_agg:8 solid_col_carry:8 solid_finish_aligned solid_report solid_seed solid_x:4 tri_setup unit_blocks untile voxelize",
        "walk", "emit_bool"),
    "bool-shard-tiled": ("bbox scan_onepass tri_setup unit_blocks untile voxelize",
        "build_bricks3 build_mip2 scan_onepass walk", "emit_bool"),
    "bool-shard-direct": ("bbox scan_onepass tri_setup unit_blocks voxelize",
        "build_bricks3 build_mip2 scan_onepass walk", "emit_bool"),
    "bool-no-triangles": ("bbox",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "vec-materials": ("bbox build_bricks3 build_mip2 emit_units mat_ids_calls mat_last scan_onepass:3 tri_setup unit_blocks voxelize",
        "walk", ""),
    "vec-solid": ("bbox brick_mip1 build_bricks3 build_mip2 emit_units scan_onepass:4 solid_col:8 solid_col_agg:8 solid_col_carry:8 solid_finish_aligned solid_report solid_seed solid_x:4 tri_setup unit_blocks untile voxelize",
        "walk", ""),
    "vec-shard-tiled": ("bbox emit_units scan_onepass:2 tri_setup unit_blocks untile voxelize",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "vec-shard-direct": ("bbox emit_units scan_onepass:2 tri_setup unit_blocks voxelize",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "vec-no-triangles": ("bbox",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "bool-words": ("bbox scan_onepass tri_setup unit_blocks untile voxelize",
        "brick_mip1 build_bricks3 build_mip2 scan_onepass walk", "emit_bool"),
    "vec-empty-range": ("bbox",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "bool-empty-range": ("bbox",
        "build_bricks3 build_mip2 scan_onepass walk", ""),
    "vec-after-failed": ("bbox build_bricks3 mip2_scan scan_onepass tri_setup unit_blocks voxelize",
        "emit_units scan_onepass walk", ""),
    "bool-after-failed": ("bbox build_bricks3 build_mip2 scan_onepass:2 tri_setup unit_blocks voxelize",
        "walk", "emit_bool"),
}.items()}
