"""Cases of the stale-memory tests (tests/test_gpu_poison.py, tests/test_gpu_stale_scratch.py); tests/test_stale_cases_cpu.py checks them
where there is no GPU.  Host data only: every library handle is made by the test that uses it.

Two grid shapes.  LARGE = 70 x 33 x 17: rows of 70 cells start at varying bit offsets of the mask words, the mask has 1228 words of which
the last holds 6 cells, and its 39 270 cells are more than two 16 384-element scan tiles.  SMALL = 9 x 7 x 5: 315 cells, 10 words, 27 live
bits in the last.  Masks are random with a fixed seed (about half of LARGE, about a tenth of SMALL), empty or full; meshes are the box
soups of tests/test_gpu_build_chain.py, whose two pinned vertices give exactly these dimensions at voxel size 1."""
import functools

import numpy as np

import solid_ref
from test_gpu_build_chain import box_soup

F = np.float32
LARGE, SMALL = (70, 33, 17), (9, 7, 5)
PATTERNS = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)
ORG, VS = (0.25, -1.0, 3.0), F(0.5)     # where the mask grids sit (exact floats at every lattice plane)
SOUP_VS = F(1.0)
SOUP_TRIS = {LARGE: 3000, SMALL: 3}


def nwords(dims):
    return (dims[0] * dims[1] * dims[2] + 31) // 32


def live_bits_of_last_word(dims):
    return (dims[0] * dims[1] * dims[2] - 1) % 32 + 1


def random_cells(dims, density, seed):
    """bool [Z, Y, X]"""
    X, Y, Z = dims
    return np.random.default_rng(seed).random((Z, Y, X)) < density


@functools.lru_cache(maxsize=None)
def mask_cases():
    """(name, bool [Z, Y, X]) of every mask the grid-analysis tests run on"""
    out = [("large_half", random_cells(LARGE, 0.5, 11)), ("small_tenth", random_cells(SMALL, 0.1, 12)),
           ("large_empty", np.zeros(LARGE[::-1], bool)), ("large_full", np.ones(LARGE[::-1], bool)),
           ("small_empty", np.zeros(SMALL[::-1], bool)), ("small_full", np.ones(SMALL[::-1], bool))]
    for _, c in out:
        c.setflags(write=False)
    return tuple(out)


def mask(name):
    return dict(mask_cases())[name]


def words_of(cells):
    return solid_ref.pack(cells)


def sparse_cells(dims, seed, n=9):
    """a handful of occupied cells far apart: large balls, long distances (the morphology's distance path, the feature transform)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    c = np.zeros((Z, Y, X), bool)
    c[rng.integers(0, Z, n), rng.integers(0, Y, n), rng.integers(0, X, n)] = True
    return c


def cavity_cells(dims=LARGE, opened=False):
    """two closed boxes (walls one cell thick) in an otherwise random sparse grid: their insides are interior cells.  opened: one wall cell
    of the first box is removed, and its inside is exterior"""
    X, Y, Z = dims
    c = random_cells(dims, 0.02, 13)
    for (x0, x1), (y0, y1), (z0, z1) in (((3, 40), (2, 20), (1, 12)), ((45, 66), (5, 30), (3, 15))):
        c[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = False
        c[z0:z1 + 1, y0:y1 + 1, [x0, x1]] = True
        c[z0:z1 + 1, [y0, y1], x0:x1 + 1] = True
        c[[z0, z1], y0:y1 + 1, x0:x1 + 1] = True
    if opened:
        c[6, 10, 3] = False
    return c


def soup(dims, seed=1):
    """(vertices, triangles) of the box soup whose grid at voxel size 1 has exactly `dims` cells"""
    return box_soup(dims, SOUP_TRIS[tuple(dims)], seed)


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def soup_ref(dims, sat=0, seed=1):
    """the oracle's builds of a box soup: computed once and left unchanged"""
    import oracle
    r = Ref()
    r.v, r.t = soup(dims, seed)
    r.words, r.calls, r.gi = oracle.build_bool(r.v, r.t, SOUP_VS, threads=0, sat=sat)
    assert tuple(r.gi["dim"]) == tuple(dims)
    r.boxes = oracle.bool_aabbs(r.words, r.gi, SOUP_VS)
    r.vec = oracle.build_vec(r.v, r.t, SOUP_VS, threads=0, sat=sat)
    r.structs, r.struct_bytes = oracle.build_aabbstruct(r.v, r.t, SOUP_VS, threads=0, sat=sat)
    r.cells = solid_ref.unpack(r.words, dims)
    return r


@functools.lru_cache(maxsize=None)
def soup_rays(dims):
    """a few hundred rays of every family through the soup's grid"""
    from test_gpu_multihit import family_rays
    r = soup_ref(dims)
    rays = family_rays(dims, r.gi["bmin"], SOUP_VS, np.argwhere(r.cells)[:, ::-1], seed=3)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def mask_ref(name):
    """a mask grid's list, its rays and the matrix of their reference hit times"""
    import multihit_ref
    import oracle
    from test_gpu_multihit import family_rays
    r = Ref()
    r.cells = mask(name)
    r.dims = r.cells.shape[::-1]
    r.gi = dict(dim=r.dims, bmin=np.asarray(ORG, F))
    r.boxes = oracle.bool_aabbs(words_of(r.cells), r.gi, VS)
    r.rays = family_rays(r.dims, ORG, VS, np.argwhere(r.cells)[:, ::-1], seed=len(name))
    r.times = multihit_ref.hit_times(r.boxes, r.rays)
    return r


def tiled(n, count):
    """indices that repeat a base set of `n` rays up to a batch of `count`: the batch's reference is the base set's, indexed"""
    return np.arange(count) % n


def kinds(gpu):
    return (gpu.GRID_BOOL, gpu.GRID_AABBSTRUCT, gpu.GRID_VEC)


def check_build(gpu, g, kind, r, what=""):
    """mask, list and counts of a build of soup `r` against the oracle"""
    d = g.describe()
    assert d["dim"] == r.gi["dim"] and d["triangles"] == len(r.t), what
    assert np.array_equal(g.bitmask(), r.words), what + ": bitmask"
    a = g.aabbs()
    if kind == gpu.GRID_VEC:
        assert a.tobytes() == r.vec.tobytes(), what + ": Vec list"
        assert d["set_calls"] == len(r.vec) and g.memory_bytes() == 24 * len(r.vec)
    elif kind == gpu.GRID_AABBSTRUCT:
        assert a.tobytes() == r.structs.tobytes(), what + ": AABBstruct list"
        assert d["set_calls"] == r.calls and g.memory_bytes() == r.struct_bytes
    else:
        assert a.tobytes() == r.boxes.tobytes(), what + ": Bool list"
        assert d["set_calls"] == r.calls and g.memory_bytes() == 4 * len(r.words)
    assert d["occupied"] == len(r.boxes), what


def check_material_ids(gpu, g, kind, r, recs, ids):
    """getMatIdx() of a VX_VOXELIZE_MATERIALS build of soup `r` against the oracle's"""
    import oracle
    from test_gpu_parity import _value_ids
    tv, nvalues, _ = _value_ids(recs, ids)
    per_call = kind == gpu.GRID_VEC
    oids, order = oracle.material_ids(r.v, r.t, SOUP_VS, tv, nvalues, per_call=per_call, ncalls=len(r.vec) if per_call else 0)
    mats, mid = g.materials()
    assert np.array_equal(mid, oids) and len(mats) == len(order), "material ids, kind %d" % kind


def material_records(gpu, ntri, k=3):
    """k material records and a per-triangle id pattern that uses all of them (and leaves some faces without one)"""
    recs = np.zeros(k, gpu.MATERIAL)
    for i in range(k):
        recs[i]["diffuse"] = (0.2 + 0.1 * i, 0.3, 0.9 - 0.2 * i)
        recs[i]["ambient"] = (0.1, 0.05 * i, 0.1)
        recs[i]["specular"] = 0.5
        recs[i]["shininess"] = 10 + i
        recs[i]["ior"], recs[i]["dissolve"], recs[i]["illum"], recs[i]["texture_id"] = 1.0, 1.0, 2, -1
    ids = (np.arange(ntri) % (k + 1) - 1).astype(np.int32)
    return recs, ids


# ---- the checks of the grid-analysis features (groups 10 to 15 of the poison tests), each against its own reference -----------------------
def write_cells(gpu, g, cells):
    """the mask of an existing grid handle, through the mutable device pointer and refresh()"""
    from test_gpu_solid import write_mask
    write_mask(g, words_of(cells))
    g.refresh()


def masked_grid(gpu, cells, kind=None):
    Z, Y, X = cells.shape
    g = gpu.Grid.create(gpu.GRID_BOOL if kind is None else kind, X, Y, Z, VS, ORG)
    write_cells(gpu, g, cells)
    return g


def check_mask(g, cells, what=""):
    w = g.bitmask()
    assert np.array_equal(w, words_of(cells)), "%s: bitmask, %d words differ" % (what, int((w != words_of(cells)).sum()))
    assert g.describe()["occupied"] == int(cells.sum()), what


def check_bool_list(g, cells, what=""):
    import oracle
    d = g.describe()
    gi = dict(dim=d["dim"], bmin=d["origin"])
    assert g.aabbs().tobytes() == oracle.bool_aabbs(words_of(cells), gi, F(d["voxel_size"])).tobytes(), what + ": AABB list"


def check_distance(g, cells, device=True):
    from test_gpu_distance import check_fields
    m = check_fields(g, device=device)[0]
    assert np.array_equal(m, cells)


def check_nearest(g, cells, device=True):
    from test_gpu_nearest import check_nearest as check
    m = check(g, device=device, gather=True)[0]
    assert np.array_equal(m, cells)


def morph_radii(gpu):
    """(radius_sq on the bit path, radius_sq just above vx_morph_bit_radius(): the distance-field path)"""
    R = gpu.morph_bit_radius() + 1
    return 5, R * R


def check_morph(gpu, g, cells, ops=None, radii=None, grids=True, what=""):
    """every operation at both radii: the mask variant, and (grids) the grid variant with its list; seal"""
    import morph_ref as mr
    ops = (mr.DILATE, mr.ERODE, mr.OPEN, mr.CLOSE) if ops is None else ops
    for r2 in (morph_radii(gpu) if radii is None else radii):
        for op in ops:
            want = mr.apply_fast(op, cells, r2, c=True)
            got = g.morph_mask(op, r2)
            assert np.array_equal(got, words_of(want)), "%s op %d r2=%d: %d words differ" % (what, op, r2, int((got != words_of(want)).sum()))
            if grids:
                r = g._morph_grid(op, None, r2)
                check_mask(r, want, "%s op %d r2=%d grid" % (what, op, r2))
                check_bool_list(r, want, "%s op %d r2=%d grid" % (what, op, r2))   # (every flavour: a result's list is its cells, ascending)
                r.free()
    if grids:
        want = mr.seal_fast(cells, 2, c=True)
        r = g.seal(radius_sq=2)
        check_mask(r, want, what + " seal")
        assert r.interior() == int(want.sum()) - int(cells.sum())
        r.free()


def check_surfaces(gpu, g, cells, materials=False, meshes=True, device=True):
    import nets_ref
    import surface_ref as sr
    from test_gpu_nets import check as check_nets
    from test_gpu_surface import check_surface
    c, want = check_surface(g, materials=materials, device=device)
    assert np.array_equal(c, cells)
    _, smooth = check_nets(gpu, g, 2, 0.5, -0.53, materials=materials, normals=True, device=device, cells=cells)
    if meshes:
        m = g.surface_mesh(materials=materials)
        v, t = m.host_arrays()
        assert v.tobytes() == want[0].tobytes() and t.tobytes() == want[1].tobytes()
        if materials and len(t):
            assert np.array_equal(m.materials()[1], want[2])
        m.free()
        m = g.surface_smooth_mesh(2, 0.5, -0.53, materials=materials, normals=True)
        v, t = m.host_arrays()
        assert v.tobytes() == smooth[0].tobytes() and t.tobytes() == smooth[1].tobytes()
        if len(t):
            assert m.corner_normals().tobytes() == smooth[-1][smooth[1]].tobytes()   # per triangle, its corners' vertex normals
        m.free()


def check_components(g, cells, device=True):
    import components_ref as cr
    import nearest_ref as nr
    from test_gpu_components import check
    _, out = check(g, device=device, cells=cells)
    near = nr.nearest_c(cells)
    for c, (lab, k) in out.items():
        got, kk = g.nearest_labels(c)
        assert kk == k
        want = np.zeros(cells.shape, np.uint32) if not k else lab.reshape(-1)[near]
        assert np.array_equal(got, want), "nearest_labels, connectivity %d" % c


def check_fill(gpu, g, cells, what=""):
    """fill_interior on the handle (changes its mask): the solid mask, the count, the list"""
    X, Y, Z = cells.shape[::-1]
    before = g.aabbs() if g.describe()["kind"] == gpu.GRID_VEC else None
    sw, hw, nh = solid_ref.fill(words_of(cells), (X, Y, Z))
    n = g.fill_interior()
    assert n == nh == g.interior(), (what, n, nh)
    assert np.array_equal(g.bitmask(), sw), what + ": solid mask"
    filled = solid_ref.unpack(sw, (X, Y, Z))
    if before is None:
        check_bool_list(g, filled, what + " filled")
    else:
        import oracle
        d = g.describe()
        gi = dict(dim=d["dim"], bmin=d["origin"])
        a = g.aabbs()
        assert a[:len(before)].tobytes() == before.tobytes() and a[len(before):].tobytes() == oracle.bool_aabbs(hw, gi, F(d["voxel_size"])).tobytes(), what
    return filled


def check_analysis(gpu, g, cells, materials=False, device=True, what=""):
    """every call of the grid-analysis features on one handle whose mask is `cells`; the fill comes last: it changes the mask"""
    check_mask(g, cells, what)
    check_distance(g, cells, device)
    check_nearest(g, cells, device)
    check_morph(gpu, g, cells, what=what)
    check_surfaces(gpu, g, cells, materials=materials, device=device)
    check_components(g, cells, device)
    return check_fill(gpu, g, cells, what)


def sliver_case():
    """the BVH case with slivers and collinear triangles (vx_scenes' `adversarial`): the ill-conditioned side list exists"""
    import mesh_multihit_cases as mc
    return mc.bvh_case("adversarial")
