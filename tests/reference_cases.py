"""Cases and helpers shared by the reference-parity tests (tests/test_reference_cpu.py, tests/test_gpu_reference.py) and the
generator of tests/golden/reference_outputs.json (tests/golden/make_reference_golden.py).

A case is a scene (vertex and triangle arrays, built here or by vx_scenes) written as an OBJ file (`v` with %.9g, which
round-trips float32 exactly, and `f` lines) plus a voxel size and a vxref mode.  `expected()` states what the CPU oracle
says the reference prints and returns for that case; the CPU tests compare it with the reference's own build (vxref)."""
import hashlib
import json
import os
import subprocess

import numpy as np

import oracle
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# oracle/_ref/vxref: the reference's own voxelizer, built from its checkout by oracle/ref/Makefile (__graft_entry__.build_ref)
VXREF = os.path.join(ROOT, "oracle", "_ref", "vxref")
REFERENCE_DIR = os.environ.get("VOXHIP_REFERENCE_DIR", "/root/reference")


def build_ref():
    """(Re)build vxref where the reference checkout exists -> True when a vxref binary is there to run."""
    import __graft_entry__
    __graft_entry__.build_ref()
    return os.path.exists(VXREF)


def run_vxref(obj, vs, mode, out_prefix, timeout=600):
    """Run vxref on an OBJ file -> dict(stdout lines, aabbs (AABB[]), occ (uint32 words; grids except Vec, else None), info)."""
    out_prefix = os.fspath(out_prefix)
    for ext in (".aabbs", ".occ", ".json"):   # no stale output of an earlier run with the same prefix
        if os.path.exists(out_prefix + ext):
            os.remove(out_prefix + ext)
    r = subprocess.run([VXREF, os.fspath(obj), "%.9g" % np.float32(vs), mode, out_prefix], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("vxref %s %s %s failed (%d): %s" % (obj, vs, mode, r.returncode, r.stderr))
    with open(out_prefix + ".json") as fh:
        info = json.load(fh)
    occ = np.fromfile(out_prefix + ".occ", dtype=np.uint32) if os.path.exists(out_prefix + ".occ") else None
    return dict(stdout=r.stdout.splitlines(), aabbs=np.fromfile(out_prefix + ".aabbs", dtype=oracle.AABB), occ=occ, info=info)

GRID_MODES = ("bool", "aabbstruct", "vec", "bool_par", "aabbstruct_par", "vec_par")
SERIAL_MODES = GRID_MODES[:3]
PAR_MODES = GRID_MODES[3:]
CUBE_SIZES = (0.5, 0.3, 0.25, 0.2, 0.1, 0.0625, 0.05)   # SURVEY.md 8(c), tests/golden/survey_anchors.json


def offset_cube():
    """The +-1 cube moved far from the origin: v - c cancels most of the mantissa."""
    return vx_scenes.cube(1.0, center=(1024.3, -517.7, 2049.1))


def flat():
    """Two triangles in the plane z = 0.5: zero extent on z -> a grid with no cells."""
    v = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def single_triangle():
    v = np.array([[0.03, 0.11, 0.07], [0.91, 0.23, 0.41], [0.37, 0.87, 0.96]], np.float32)
    return v, np.array([[0, 1, 2]], np.int32)


def no_faces():
    """Vertices only: a grid with cells and no triangle."""
    return vx_scenes.rotated_cube()[0], np.zeros((0, 3), np.int32)


def lattice(step, seed, offset=0.0, ntri=200):
    """Triangles whose vertices are float32(k * step) + offset, k in 0..11, voxelized at voxel size step: the bbox and the
    triangle extents sit on (non-dyadic) lattice planes, where (triMax - gridMin) / voxelSize rounds to either side of an
    integer -- the cases the `+ 2` of the candidate range (VoxelBuilder.hpp:171-176) exists for (an offset away from 0
    makes the subtraction round)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 12, size=(ntri * 3, 3)).astype(np.float32)
    v = (k * np.float32(step)).astype(np.float32) + np.float32(offset)
    return np.ascontiguousarray(v, dtype=np.float32), np.arange(3 * ntri, dtype=np.int32).reshape(-1, 3)


def random_soup(seed):
    """One case of the seeded sweep -> (v, t, voxel size): odd seeds are random soups (a few hundred random triangles of
    random size) at a random voxel size, even seeds lattice scenes at a random non-dyadic step."""
    rng = np.random.default_rng(1000 + seed)
    if seed % 2 == 0:
        step = np.float32(rng.choice([0.1, 0.3, 0.07, 0.013, 0.2, 0.15, 0.11]))
        v, t = lattice(step, 3000 + seed, offset=float(rng.choice([0.37, -5.1, 1.3])), ntri=int(rng.integers(1, 300)))
        return v, t, step
    ntri = int(rng.integers(1, 300))
    edge = float(rng.uniform(0.005, 0.4))
    v, t = vx_scenes.soup(ntri, seed=2000 + seed, edge=edge, extent=float(rng.uniform(0.5, 2.0)))
    return v, t, np.float32(rng.uniform(0.02, 0.25))


SCENES = {
    "offsetcube": offset_cube,
    "flat": flat,
    "single": single_triangle,
    "nofaces": no_faces,
    "lattice01": lambda: lattice(0.1, 6, 0.37),      # voxelized at 0.1
    "lattice02": lambda: lattice(0.2, 0, -5.1),      # at 0.2
    "lattice007": lambda: lattice(0.07, 0, -5.1),    # at 0.07
}


def scene(name):
    """(vertices float32[V, 3], triangles int32[T, 3]) of a named case scene."""
    if name in SCENES:
        return SCENES[name]()
    if name.startswith("rsoup"):
        v, t, _ = random_soup(int(name[5:]))
        return v, t
    if name == "atrium":
        return vx_scenes.scene("atrium262k")
    return vx_scenes.scene(name)


def write_obj(path, v, t, negative=False):
    """%.9g vertices; 1-based face indices, or (negative=True) indices relative to the end of the vertex list so far,
    each triangle written right after its own vertices."""
    v = np.asarray(v, np.float32)
    t = np.asarray(t, np.int64)
    if not negative:
        vx_scenes.write_obj(str(path), v, t)
        return
    with open(path, "w") as fh:
        fh.write("# negative (relative) face indices\n")
        for tri in t.tolist():
            for k in tri:
                fh.write("v %.9g %.9g %.9g\n" % tuple(v[k].tolist()))
            fh.write("f -3 -2 -1\n")


def negative_index_mesh(v, t):
    """The mesh an OBJ from write_obj(..., negative=True) describes: three fresh vertices per triangle."""
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(v[np.asarray(t, np.int64).reshape(-1)]), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sorted_sha(aabbs):
    """Hash of the boxes sorted by their 24 raw bytes: equal for two lists that are the same multiset."""
    a = np.ascontiguousarray(aabbs, dtype=oracle.AABB)
    return sha(np.sort(a.view(np.dtype((np.void, 24))).reshape(-1)))


def fmt_float(x):
    """std::format("{}", float) == std::to_chars(first, last, value): the shortest digits that round-trip, in fixed or
    scientific notation, whichever is shorter (fixed on a tie); the exponent has a sign and at least two digits."""
    x = np.float32(x)
    if np.isnan(x):
        return "-nan" if np.signbit(x) else "nan"
    if np.isinf(x):
        return "-inf" if x < 0 else "inf"
    sign = "-" if np.signbit(x) else ""
    if x == 0:
        return sign + "0"
    mant, exp = np.format_float_scientific(abs(x), unique=True, trim="-").split("e")
    digits, exp = mant.replace(".", ""), int(exp)
    sci = digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e" + ("-" if exp < 0 else "+") + "%02d" % abs(exp)
    if exp >= 0:
        ip = digits[:exp + 1].ljust(exp + 1, "0")
        fp = digits[exp + 1:]
        fixed = ip + ("." + fp if fp else "")
    else:
        fixed = "0." + "0" * (-exp - 1) + digits
    return sign + (fixed if len(fixed) <= len(sci) else sci)


def stdout_lines(v, t, vs, mode, threads, n_items=None, n_nodes=None):
    """The lines the reference prints for this case (VoxelBuilder.hpp:343-352, 417, 440-464; octTree.hpp:568-808), with
    the values the oracle computes."""
    gi = oracle.grid_info(v, vs)
    ntri = len(t)
    dims = "Grid dimensions: %dx%dx%d" % gi["dim"]
    vsz = "Voxel size: " + fmt_float(vs)
    using = "Using %d threads for voxelization over %d triangles." % (threads, ntri)
    if mode.startswith("octree"):
        out = [dims, vsz]
        if max(gi["dim"]) == 0:
            return out + ["Empty voxel grid (zero extent)."]
        if ntri == 0:
            return out + ["No triangles in OBJ, nothing to voxelize."]
        return out + [using, "Total triangles processed: %d" % ntri, "Total voxels inserted (before tree build): %d" % n_items,
                      "Total octree nodes: %d" % n_nodes]
    out = ["Bounding box: %s(%s):" % (k, ",".join(fmt_float(c) for c in gi[g])) for k, g in
           (("min", "bmin"), ("max", "bmax"), ("center", "center"))]
    out += [dims, vsz]
    if mode.endswith("_par"):
        if ntri == 0:
            return out + ["No triangles in OBJ, nothing to voxelize."]
        out.append(using)
    return out + ["Total triangles processed: %d" % ntri]


def max_items_of(mode):
    return int(mode.split(":")[1]) if ":" in mode else 16


def expected(v, t, vs, mode, threads):
    """What the oracle says vxref writes for this case: dict(stdout, aabbs, occ (None for vec / octree), memory_bytes,
    calls (setVoxel calls; grids only)).  threads: the reference's thread count (its parallel paths only)."""
    vs = np.float32(vs)
    if mode.startswith("octree"):
        oc = oracle.octree(v, t, vs, max_items=max_items_of(mode), threads=threads)
        return dict(stdout=stdout_lines(v, t, vs, mode, threads, len(oc["items"]), len(oc["nodes"])), aabbs=oc["aabbs"], occ=None,
                    memory_bytes=oc["bytes"], calls=None)
    th = threads if mode.endswith("_par") else 0     # threaded driver + SAT a8 / serial driver + SAT a7
    words, calls, gi = oracle.build_bool(v, t, vs, threads=th)
    kind = mode.split("_")[0]
    if kind == "bool":
        aabbs, mem = oracle.bool_aabbs(words, gi, vs), 4 * len(words)
    elif kind == "aabbstruct":
        aabbs, mem = oracle.build_aabbstruct(v, t, vs, threads=th)
    else:
        aabbs = oracle.build_vec(v, t, vs, threads=th)
        mem = 24 * len(aabbs)
    return dict(stdout=stdout_lines(v, t, vs, mode, threads), aabbs=aabbs, occ=None if kind == "vec" else words, memory_bytes=mem,
                calls=calls)


def threads_of(stdout):
    """N of the reference's `Using N threads for voxelization over T triangles.` line (None when it printed none)."""
    for line in stdout:
        if line.startswith("Using ") and " threads for voxelization" in line:
            return int(line.split()[1])
    return None
