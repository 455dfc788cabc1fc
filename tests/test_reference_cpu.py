"""The CPU oracle (oracle/vx_oracle.c) against the reference's own voxelizer, built from its sources (oracle/_ref/vxref,
`make -C oracle ref`): AABB list bytes, occupancy, Vec order with duplicates, setVoxel-call count, octree list and
memory bytes, and the reference's stdout lines, character for character, for both drivers and both SAT variants.

The reference's parallel paths split the triangles over std::thread::hardware_concurrency() threads; the tests read that
N from its `Using N threads` line and run the oracle's threaded driver with the same N, so the Vec order must match too.
Skipped only where neither the reference sources nor a built vxref exist."""
import os

import numpy as np
import pytest

import oracle
import reference_cases as rc


@pytest.fixture(scope="module")
def vxref():
    if not rc.build_ref():
        pytest.skip("no reference voxelizer: neither the reference sources (VOXHIP_REFERENCE_DIR=%s) nor a built %s exist"
                    % (rc.REFERENCE_DIR, rc.VXREF))
    return rc.VXREF


def check(tmp_path, v, t, vs, mode, obj=None):
    """Run vxref on the case and compare everything it writes with the oracle.  -> the reference's thread count (or None)."""
    vs = np.float32(vs)
    if obj is None:
        obj = tmp_path / "scene.obj"
        if not obj.exists():
            rc.write_obj(obj, v, t)
    r = rc.run_vxref(obj, vs, mode, tmp_path / ("out_" + mode.replace(":", "_")))
    n = rc.threads_of(r["stdout"])
    e = rc.expected(v, t, vs, mode, n or 1)
    what = "%s at %.9g" % (mode, vs) + (" (reference threads N=%d)" % n if n else "")
    assert r["stdout"] == e["stdout"], what
    assert r["aabbs"].tobytes() == e["aabbs"].tobytes(), "%s: AABB list differs (%d vs %d boxes)" % (what, len(r["aabbs"]), len(e["aabbs"]))
    if e["occ"] is not None:
        assert np.array_equal(r["occ"], e["occ"]), what + ": occupancy differs"
    assert r["info"]["memory_bytes"] == e["memory_bytes"], what
    if mode.startswith("vec"):
        assert len(r["aabbs"]) == e["calls"], what + ": setVoxel calls"     # one Vec entry per setVoxel call
    if r["info"]["dims"] is not None:
        assert tuple(r["info"]["dims"]) == oracle.grid_info(v, vs)["dim"], what
    if n:
        print("%s: reference threads N=%d" % (what, n))
    return n


ALL_MODES = rc.GRID_MODES + ("octree",)

SCENE_CASES = ([("cube", vs) for vs in rc.CUBE_SIZES] +
               [("rotcube", 0.09), ("rotcube", 0.031), ("adversarial", 0.125), ("adversarial", 0.1), ("adversarial", 0.0625),
                ("soup2000", 0.02), ("blob70k", 2.0 / 64), ("blob70k", 2.0 / 128), ("atrium", 32.0 / 64),
                ("offsetcube", 0.1), ("offsetcube", 0.0625), ("flat", 0.125), ("single", 0.05), ("nofaces", 0.25),
                ("lattice01", 0.1), ("lattice02", 0.2), ("lattice007", 0.07)])


@pytest.mark.parametrize("name,vs", SCENE_CASES, ids=["%s@%.6g" % c for c in SCENE_CASES])
def test_scene_all_modes(vxref, tmp_path, name, vs):
    """Every flavour (Bool / AABBstruct / Vec, serial and parallel, octree) on the named scenes."""
    v, t = rc.scene(name)
    for mode in ALL_MODES:
        check(tmp_path, v, t, vs, mode)


def test_survey_anchors_from_the_reference(vxref, tmp_path):
    """tests/golden/survey_anchors.json re-derived from the live reference."""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "survey_anchors.json")) as fh:
        A = json.load(fh)["cube_pm1"]
    v, t = rc.scene("cube")
    obj = tmp_path / "cube.obj"
    rc.write_obj(obj, v, t)
    for i, vs in enumerate(A["voxel_sizes"]):
        assert len(rc.run_vxref(obj, vs, "bool", tmp_path / "b")["aabbs"]) == A["bool_occupied"][i]
        assert len(rc.run_vxref(obj, vs, "vec", tmp_path / "v")["aabbs"]) == A["vec_items"][i]
        oc = rc.run_vxref(obj, vs, "octree", tmp_path / "o")
        assert len(oc["aabbs"]) == A["octree_items"][i]
        if vs == 0.25:
            assert oc["info"]["memory_bytes"] == A["octree_bytes_at_0.25"]
            assert "Total octree nodes: %d" % A["octree_nodes_at_0.25"] in oc["stdout"]


@pytest.mark.parametrize("max_items", [1, 3, 16, 64, 65])
@pytest.mark.parametrize("name,vs", [("rotcube", 0.09), ("soup2000", 0.02), ("adversarial", 0.0625)])
def test_octree_max_items(vxref, tmp_path, name, vs, max_items):
    """Octree(path, vs, maxItemsPerLeaf): leaf order of getAabbs, node count (stdout) and getMemoryUsageBytes."""
    v, t = rc.scene(name)
    check(tmp_path, v, t, vs, "octree:%d" % max_items)


def test_negative_indices(vxref, tmp_path):
    """`f -3 -2 -1` after each triangle's vertices: the OBJ indices are relative to the vertices read so far."""
    v, t = rc.scene("rotcube")
    obj = tmp_path / "neg.obj"
    rc.write_obj(obj, v, t, negative=True)
    mv, mt = rc.negative_index_mesh(v, t)
    for mode in ALL_MODES:
        check(tmp_path, mv, mt, 0.09, mode, obj=obj)


@pytest.mark.parametrize("seed", range(30))
def test_random_soup_sweep(vxref, tmp_path, seed):
    """Seeded random soups at random voxel sizes through both drivers (SAT triBoxOverlap and triBoxOverlapSchwarzSeidel)."""
    v, t, vs = rc.random_soup(seed)
    for mode in ("bool", "vec", "bool_par", "vec_par", "octree"):
        check(tmp_path, v, t, vs, mode)


def _golden():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.json")) as fh:
        return json.load(fh)["entries"]


def _with_threads(lines, n):
    """The stdout lines with the reference's thread count replaced by n (it is the generating machine's CPU count)."""
    return [("Using %d threads" % n + l[l.index(" threads") + 8:]) if l.startswith("Using ") else l for l in lines]


def test_oracle_reproduces_reference_golden():
    """tests/golden/reference_outputs.json (written by the reference built from its sources): the oracle reproduces every
    entry without the reference present -- list and occupancy hashes, counts, memory bytes and stdout lines."""
    scenes = {}
    for g in _golden():
        if g["scene"] not in scenes:
            scenes[g["scene"]] = rc.scene(g["scene"])
        v, t = scenes[g["scene"]]
        e = rc.expected(v, t, np.float32(g["voxel_size"]), g["mode"], g.get("threads") or 1)
        what = "%s %s at %s" % (g["scene"], g["mode"], g["voxel_size"])
        assert rc.sha(e["aabbs"]) == g["aabbs_sha"] and len(e["aabbs"]) == g["num_aabbs"], what
        assert (None if e["occ"] is None else rc.sha(e["occ"])) == g["occ_sha"], what
        assert e["memory_bytes"] == g["memory_bytes"], what
        assert e["stdout"] == g["stdout"], what
        if "sorted_aabbs_sha" in g:
            assert rc.sorted_sha(e["aabbs"]) == g["sorted_aabbs_sha"], what


def test_vxref_reproduces_reference_golden(vxref, tmp_path):
    """Drift guard on the stand-in headers: today's vxref still writes every committed entry."""
    objs = {}
    for g in _golden():
        if g["scene"] not in objs:
            objs[g["scene"]] = tmp_path / (g["scene"] + ".obj")
            rc.write_obj(objs[g["scene"]], *rc.scene(g["scene"]))
        r = rc.run_vxref(objs[g["scene"]], np.float32(g["voxel_size"]), g["mode"], tmp_path / "out")
        what = "%s %s at %s" % (g["scene"], g["mode"], g["voxel_size"])
        n = rc.threads_of(r["stdout"])
        assert r["stdout"] == (_with_threads(g["stdout"], n) if n else g["stdout"]), what
        assert rc.sha(r["aabbs"]) == g["aabbs_sha"] and len(r["aabbs"]) == g["num_aabbs"], what
        assert (None if r["occ"] is None else rc.sha(r["occ"])) == g["occ_sha"], what
        assert r["info"]["memory_bytes"] == g["memory_bytes"], what
