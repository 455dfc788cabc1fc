"""Regenerates tests/golden/reference_outputs.json: what the reference's own voxelizer (oracle/_ref/vxref, built from its
sources by `make -C oracle ref`) writes and prints for a fixed set of cases (tests/reference_cases.py).

Per entry: sha256 of the getAabbs() bytes and of the occupancy words read through getVoxel, the box count,
getMemoryUsageBytes(), and the stdout lines verbatim.  Parallel-driver entries also record the thread count N the reference
used (its `Using N threads` line), a hash of the boxes sorted by their bytes (the list as a multiset) and whether the
parallel list equals the serial driver's list in order.  tests/test_reference_cpu.py checks that the oracle and vxref still
reproduce every entry; tests/test_gpu_reference.py checks the GPU against them.

    python tests/golden/make_reference_golden.py          (needs the reference checkout or a built oracle/_ref/vxref)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "raytracing-voxilizer-vulkan-intresection_amd")]
import numpy as np  # noqa: E402

import reference_cases as rc  # noqa: E402

OUT = os.path.join(HERE, "reference_outputs.json")

CASES = [("cube", 0.25), ("cube", 0.1), ("cube", 0.0625), ("rotcube", 0.09), ("adversarial", 0.125), ("adversarial", 0.1),
         ("soup2000", 0.02), ("blob70k", 2.0 / 64), ("offsetcube", 0.0625), ("single", 0.05), ("flat", 0.125),
         ("lattice02", 0.2), ("lattice007", 0.07)]
MODES = rc.GRID_MODES + ("octree",)
EXTRA = [("rotcube", 0.09, "octree:%d" % k) for k in (1, 3, 64, 65)]


def generate():
    if not rc.build_ref():
        sys.exit("no %s: the reference checkout is needed to regenerate the golden" % rc.VXREF)
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, vs, modes in [(n, v, MODES) for n, v in CASES] + [(n, v, (m,)) for n, v, m in EXTRA]:
            vs = np.float32(vs)
            v, t = rc.scene(name)
            obj = os.path.join(tmp, name + ".obj")
            rc.write_obj(obj, v, t)
            runs = {m: rc.run_vxref(obj, vs, m, os.path.join(tmp, "out")) for m in modes}
            for m, r in runs.items():
                e = dict(scene=name, voxel_size="%.9g" % vs, mode=m, num_aabbs=len(r["aabbs"]), aabbs_sha=rc.sha(r["aabbs"]),
                         occ_sha=None if r["occ"] is None else rc.sha(r["occ"]), memory_bytes=r["info"]["memory_bytes"],
                         stdout=r["stdout"])
                if m.endswith("_par") or m.startswith("octree"):
                    e["threads"] = rc.threads_of(r["stdout"])
                if m.endswith("_par"):
                    e["sorted_aabbs_sha"] = rc.sorted_sha(r["aabbs"])
                    e["order_equals_serial"] = r["aabbs"].tobytes() == runs[m[:-4]]["aabbs"].tobytes()
                entries.append(e)
    doc = dict(generator="tests/golden/make_reference_golden.py",
               note="outputs of the reference's own VoxelBuilder / VoxelGrid* / Octree built from its sources (oracle/_ref/vxref); "
                    "threads = the reference's std::thread::hardware_concurrency() where the generator ran",
               entries=entries)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote %d entries to %s" % (len(entries), OUT))


if __name__ == "__main__":
    generate()
