"""bench.py --dump-outputs without a GPU: dtypes, the row sample of long outputs and the size bound of the dump."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def outputs(nrays, naabbs, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 10, nrays).astype(np.float32)
    prim = np.where(t > 0, rng.integers(0, 1 << 31, nrays), 0xFFFFFFFF).astype(np.uint32)
    lo = rng.uniform(0, 1, (naabbs, 3)).astype(np.float32)
    return t, prim, np.concatenate([lo, lo + np.float32(0.25)], axis=1).reshape(-1), naabbs


def load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


def test_dump_small_outputs_whole(tmp_path):
    t, prim, aabbs, n = outputs(1000, 700)
    names = bench.dump_outputs(str(tmp_path), t, prim, aabbs, n)
    assert names == ["aabbs", "aabbs_count", "prim", "t"]
    got = load(str(tmp_path))
    assert sorted(got) == names
    assert got["t"].dtype == np.float32 and got["t"].tobytes() == t.tobytes()
    assert got["prim"].dtype == np.float64 and np.array_equal(got["prim"], prim.astype(np.float64)) and got["prim"].max() == 0xFFFFFFFF
    assert got["aabbs"].dtype == np.float32 and got["aabbs"].shape == (700, 6) and got["aabbs"].tobytes() == aabbs.tobytes()
    assert got["aabbs_count"].dtype == np.float64 and got["aabbs_count"].tolist() == [700.0]


def test_dump_long_outputs_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    t, prim, aabbs, n = outputs(1000, 500)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert bench.dump_outputs(a, t, prim, aabbs, n) == ["aabbs", "aabbs_count", "aabbs_index", "prim", "rays_index", "t"]
    bench.dump_outputs(b, t, prim, aabbs, n)
    ga, gb = load(a), load(b)
    for k in ga:   # the sample is fixed: the same rows on every run
        assert ga[k].dtype in (np.float32, np.float64) and ga[k].tobytes() == gb[k].tobytes(), k
    ri, ai = ga["rays_index"].astype(np.int64), ga["aabbs_index"].astype(np.int64)
    assert len(ri) == len(ai) == 64 and np.all(np.diff(ri) > 0) and np.all(np.diff(ai) > 0) and ri[-1] < 1000 and ai[-1] < 500
    assert ga["t"].tobytes() == t[ri].tobytes() and np.array_equal(ga["prim"], prim[ri].astype(np.float64))
    assert ga["aabbs"].tobytes() == aabbs.reshape(-1, 6)[ai].tobytes() and ga["aabbs_count"].tolist() == [500.0]
    # a later dump of short outputs into the same directory leaves no index of the earlier rows behind
    monkeypatch.setattr(bench, "DUMP_ROWS", 1 << 20)
    bench.dump_outputs(a, t, prim, aabbs, n)
    assert sorted(os.listdir(a)) == ["aabbs.npy", "aabbs_count.npy", "prim.npy", "t.npy"]


def test_dump_bound():
    """Largest dump: DUMP_ROWS rays (t f32, prim f64, index f64) and DUMP_ROWS records (6 x f32, index f64), plus headers."""
    assert bench.DUMP_ROWS * ((4 + 8 + 8) + (24 + 8)) + 6 * 4096 <= 64_000_000
