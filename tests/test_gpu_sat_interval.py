"""k_voxelize's row interval (sat_row_interval; DESIGN.md, K2 notes, "Row interval") on the GPU: long rows sweep only the x interval their
plane test allows, and nothing the build leaves may change.  Meshes of one to three large triangles among 200 tiny ones -- so that wave
passes mix long and short rows -- on grids whose rows are whole words (64^3, 96^3, 160^3: the tiled build mask) and on one with X = 70
(the direct form); both SAT variants; GRID_BOOL and GRID_VEC; one word shard; one asynchronous rebuild followed by a trace.  The bitmask,
set_calls, the Vec list and the Bool list are compared with the oracle bit for bit."""
import numpy as np
import pytest

import oracle
import vx_scenes

pytestmark = pytest.mark.gpu

F = np.float32
VS = F(1.0 / 16)            # dyadic: the two pin triangles give the grid exactly the dims asked for
GRIDS = [(64, 64, 64), (96, 96, 96), (160, 160, 160), (70, 64, 64)]

# large triangles, in units of the grid's extent per axis
LARGE = {
    # tilted x-facing walls, like the bench scene's (normal about (1, -0.11, 0.012)), leaning both ways
    "tilted": [[(0.30, 0.02, 0.03), (0.40, 0.95, 0.05), (0.36, 0.50, 0.97)], [(0.74, 0.03, 0.04), (0.63, 0.96, 0.10), (0.70, 0.40, 0.95)]],
    # near 45 degrees in all three axes
    "diagonal": [[(0.05, 0.10, 0.90), (0.90, 0.05, 0.10), (0.50, 0.95, 0.60)], [(0.10, 0.10, 0.10), (0.90, 0.92, 0.15), (0.15, 0.90, 0.93)],
                 [(0.95, 0.05, 0.95), (0.05, 0.50, 0.05), (0.60, 0.95, 0.50)]],
    # the normal's x component tiny: almost a plane of constant y
    "nx_tiny": [[(0.05, 0.50, 0.10), (0.95, 0.50001, 0.20), (0.50, 0.500004, 0.90)], [(0.10, 0.2500, 0.85), (0.90, 0.25002, 0.80), (0.45, 0.25001, 0.10)]],
    # ... and exactly zero: planes of constant y and of constant z
    "nx_zero": [[(0.05, 0.513, 0.10), (0.95, 0.513, 0.20), (0.50, 0.513, 0.90)], [(0.10, 0.15, 0.771), (0.90, 0.30, 0.771), (0.45, 0.95, 0.771)]],
    "sliver": [[(0.05, 0.10, 0.10), (0.95, 0.90, 0.85), (0.0501, 0.1001, 0.1002)], [(0.90, 0.10, 0.50), (0.10, 0.80, 0.52), (0.1002, 0.8001, 0.5201)]],
    # zero area: three collinear vertices, and one vertex twice
    "degenerate": [[(0.10, 0.10, 0.10), (0.50, 0.50, 0.50), (0.90, 0.90, 0.90)], [(0.20, 0.80, 0.30), (0.20, 0.80, 0.30), (0.85, 0.15, 0.70)]],
}
KINDS = list(LARGE) + ["offset"]


def mesh_for(kind, dims):
    """-> verts, tris: two pin triangles at the corners of the box [0, dims * VS], 200 tiny triangles, the large ones"""
    rng = np.random.default_rng(1000 + 17 * KINDS.index(kind) + dims[0])
    ext = np.array(dims, np.float64) * float(VS)
    tris = []
    e = float(VS) / 4
    tris.append(np.array([(0, 0, 0), (e, 0, 0), (0, e, e)]))
    tris.append(ext - np.array([(0, 0, 0), (e, 0, 0), (0, e, e)]))
    c = rng.uniform(0.05, 0.95, (200, 1, 3)) * ext
    tris += list(c + rng.uniform(-0.75, 0.75, (200, 3, 3)) * float(VS))
    large = LARGE["tilted" if kind == "offset" else kind]
    tris += [np.array(t, np.float64) * ext for t in large]
    order = rng.permutation(len(tris))              # the large ones somewhere among the small ones
    v = np.concatenate([tris[i] for i in order]).astype(F)
    if kind == "offset":                            # 10^4 voxel sizes away from the origin (625: the pins stay exact)
        v = (v + F(1.0e4 * float(VS))).astype(F)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, t


_REF = {}


def reference(kind, dims, sat):
    """the oracle's build of one mesh, computed once and shared"""
    key = (kind, dims, sat)
    if key not in _REF:
        v, t = mesh_for(kind, dims)
        ow, calls, gi = oracle.build_bool(v, t, VS, threads=0, sat=sat)
        _REF[key] = dict(v=v, t=t, words=ow, calls=calls, gi=gi, bool_list=oracle.bool_aabbs(ow, gi, VS), vec_list=oracle.build_vec(v, t, VS, threads=0, sat=sat))
    return _REF[key]


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("kind", KINDS)
def test_build_matches_the_oracle(gpu, kind, dims):
    for sat in (0, 1):
        ref = reference(kind, dims, sat)
        assert ref["gi"]["dim"] == dims
        mesh = gpu.Mesh.from_arrays(ref["v"], ref["t"])
        g = gpu.Grid.voxelize(mesh, VS, gpu.GRID_BOOL, sat_variant=sat)
        d = g.describe()
        assert d["dim"] == dims and d["set_calls"] == ref["calls"], (sat, d["set_calls"], ref["calls"])
        w = g.bitmask()
        assert np.array_equal(w, ref["words"]), "sat %d: %d differing words" % (sat, int((w != ref["words"]).sum()))
        assert g.aabbs().tobytes() == ref["bool_list"].tobytes(), sat
        gv = gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC, sat_variant=sat)
        assert gv.describe()["set_calls"] == len(ref["vec_list"])
        assert gv.aabbs().tobytes() == ref["vec_list"].tobytes(), sat
        assert np.array_equal(gv.bitmask(), ref["words"])
        g.free()
        gv.free()


@pytest.mark.parametrize("dims", [GRIDS[1], GRIDS[3]], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("kind", KINDS)
def test_word_shard(gpu, kind, dims):
    """a shard that begins and ends inside a plane of the grid: its words are the oracle's, the others stay zero"""
    for sat in (0, 1):
        ref = reference(kind, dims, sat)
        n = ref["words"].size
        b, e = n // 3 + 5, (2 * n) // 3 + 11
        mesh = gpu.Mesh.from_arrays(ref["v"], ref["t"])
        g = gpu.Grid.voxelize(mesh, VS, words=(b, e), sat_variant=sat)
        w = g.bitmask()
        assert not w[:b].any() and not w[e:].any()
        assert np.array_equal(w[b:e], ref["words"][b:e]) and ref["words"][b:e].any()
        g.free()


@pytest.mark.parametrize("kind", KINDS)
def test_async_rebuild_then_trace(gpu, kind):
    """revoxelize(..., list_async=True) over a grid that held another mesh, a ray batch, then the list: the oracle's, byte for byte"""
    dims = GRIDS[1]
    other = reference("diagonal" if kind != "diagonal" else "tilted", dims, 0)
    for sat in (0, 1):
        ref = reference(kind, dims, sat)
        mesh = gpu.Mesh.from_arrays(ref["v"], ref["t"])
        rays = vx_scenes.random_rays(4096, ref["gi"]["bmin"], ref["gi"]["bmax"], seed=5)
        fresh = gpu.Grid.voxelize(mesh, VS, gpu.GRID_VEC, sat_variant=sat)
        t_ref, p_ref, _ = fresh.trace(rays)
        g = gpu.Grid.voxelize(gpu.Mesh.from_arrays(other["v"], other["t"]), VS, gpu.GRID_VEC)
        g.revoxelize(mesh, VS, sat_variant=sat, list_async=True)
        tt, pp, _ = g.trace(rays)
        assert np.array_equal(tt, t_ref) and np.array_equal(pp, p_ref)
        assert (t_ref > 0).any()
        assert g.aabbs().tobytes() == ref["vec_list"].tobytes(), sat
        assert np.array_equal(g.bitmask(), ref["words"]) and g.describe()["set_calls"] == ref["calls"]
        g.free()
        fresh.free()
