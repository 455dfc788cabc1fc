"""The GPU voxelizer against tests/golden/reference_outputs.json: outputs of the reference's own VoxelBuilder / VoxelGrid* /
Octree built from its sources (tests/golden/make_reference_golden.py).  Nothing here runs or reads the reference.

Serial entries (triBoxOverlap) run with sat_variant=0: Bool / AABBstruct / Vec lists, the Bool occupancy words and
vx_octree_aabbs hash-equal the entry.  Parallel entries (triBoxOverlapSchwarzSeidel) run with sat_variant=1: the Bool and
AABBstruct lists hash-equal the entry; the GPU emits the Vec list in serial order, so it must equal the reference's as a
multiset, and in order wherever the golden records that the reference's parallel order equals its serial order.
The `voxilizer` CLI must print the reference's lines verbatim (its own `Using MI355X ...` line stands where the reference
prints its thread count)."""
import json
import os
import subprocess

import numpy as np
import pytest

import reference_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")
with open(os.path.join(ROOT, "tests", "golden", "reference_outputs.json")) as _fh:
    GOLDEN = json.load(_fh)["entries"]
CASES = sorted({(g["scene"], g["voxel_size"]) for g in GOLDEN}, key=lambda c: [g["scene"] for g in GOLDEN].index(c[0]))


def _entries(scene, vs):
    return {g["mode"]: g for g in GOLDEN if g["scene"] == scene and g["voxel_size"] == vs}


@pytest.mark.parametrize("scene,vs", CASES, ids=["%s@%s" % c for c in CASES])
def test_gpu_matches_reference_golden(gpu, scene, vs):
    v, t = rc.scene(scene)
    vsf = np.float32(vs)
    mesh = gpu.Mesh.from_arrays(v, t)
    kinds = {"bool": gpu.GRID_BOOL, "aabbstruct": gpu.GRID_AABBSTRUCT, "vec": gpu.GRID_VEC}
    for mode, g in _entries(scene, vs).items():
        what = "%s %s at %s" % (scene, mode, vs)
        if mode.startswith("octree"):
            o = gpu.Octree(mesh, vsf, rc.max_items_of(mode))
            a = o.aabbs()
            assert rc.sha(a) == g["aabbs_sha"] and len(a) == g["num_aabbs"], what
            assert o.memory_bytes() == g["memory_bytes"], what
            continue
        par = mode.endswith("_par")
        kind = mode.split("_")[0]
        grid = gpu.Grid.voxelize(mesh, vsf, kinds[kind], sat_variant=1 if par else 0)
        a = grid.aabbs()
        assert len(a) == g["num_aabbs"] and grid.memory_bytes() == g["memory_bytes"], what
        if kind == "bool" and g["occ_sha"] is not None:
            assert rc.sha(grid.bitmask()) == g["occ_sha"], what + ": occupancy words"
        if kind == "vec" and par:
            assert rc.sorted_sha(a) == g["sorted_aabbs_sha"], what + ": Vec multiset (reference threads N=%s)" % g["threads"]
            if g["order_equals_serial"]:
                assert rc.sha(a) == g["aabbs_sha"], what + ": Vec order"
        else:
            assert rc.sha(a) == g["aabbs_sha"], what


CLI_CASES = [c for c in CASES if c[0] in ("cube", "rotcube", "offsetcube", "lattice02", "single", "flat")]


@pytest.mark.parametrize("scene,vs", CLI_CASES, ids=["%s@%s" % c for c in CLI_CASES])
def test_cli_prints_reference_lines(gpu, tmp_path, scene, vs):
    """voxilizer <obj> <vs> [--grid ...] [--parallel]: every line the reference printed for the entry, verbatim, in order."""
    obj = tmp_path / "scene.obj"
    rc.write_obj(obj, *rc.scene(scene))
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    for mode, g in _entries(scene, vs).items():
        args = ["--grid", mode.split("_")[0].split(":")[0]] + (["--parallel"] if mode.endswith("_par") else [])
        if ":" in mode:
            continue       # the CLI builds the octree with the default 16 items per leaf
        r = subprocess.run([os.path.join(PKG, "voxilizer"), str(obj), vs] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout
        want = [line for line in g["stdout"] if not line.startswith("Using ")]
        got = [line for line in r.stdout.splitlines() if line in want]
        assert got == want, "%s %s: reference lines %s\nCLI printed\n%s" % (scene, mode, want, r.stdout)
