"""tests/scan_ref.py against brute-force loops in plain Python integers (no GPU): the exclusive prefix, the 32-bit outputs, the total
contract and every caller's refusal, sel and group16, on small and adversarial arrays."""
import numpy as np
import pytest

import scan_ref as sr

M32 = 1 << 32


def brute(x, mode):
    f = {"values": int, "popcount": lambda w: bin(int(w)).count("1"), "bytes": int}[mode]
    p, acc = [0], 0
    for e in x:
        acc += f(e)
        p.append(acc)
    return p


ARRAYS = {
    "empty": np.zeros(0, np.uint32),
    "one": np.array([7], np.uint32),
    "zeros17": np.zeros(17, np.uint32),
    "ones15": np.ones(15, np.uint32),
    "pair_2^31": np.array([1 << 31, 1 << 31], np.uint32),
    "pair_below": np.array([(1 << 31) - 1, 1 << 31], np.uint32),
    "pair_above": np.array([1 << 31, (1 << 31) + 1], np.uint32),
    "full": np.full(33, 0xFFFFFFFF, np.uint32),
    "huge_last": np.concatenate([np.arange(40, dtype=np.uint32), [0xFFFFFFFF]]).astype(np.uint32),
    "random": np.random.default_rng(1).integers(0, M32, 200, dtype=np.uint64).astype(np.uint32),
}


@pytest.mark.parametrize("name", sorted(ARRAYS))
@pytest.mark.parametrize("mode", ["values", "popcount", "bytes"])
def test_exclusive_and_outputs(name, mode):
    x = ARRAYS[name]
    if mode == "bytes":
        x = x.view(np.uint8)
    p = sr.exclusive(x, mode)
    b = brute(x, mode)
    assert [int(v) for v in p] == b
    assert [int(v) for v in sr.outputs(p)] == [v % M32 for v in b]
    assert sr.defined(p).all()


def test_defined_tiles():
    """a tile's outputs are specified while its exclusive prefix is below SAT: all-0xFFFFFFFF passes 2^40 inside tile 0."""
    x = np.full(3 * sr.TILE + 5, 0xFFFFFFFF, np.uint32)
    d = sr.defined(sr.exclusive(x))
    assert d.size == x.size + 1 and d[: sr.TILE].all() and not d[sr.TILE:].any()
    y = np.full(2 * sr.TILE, 1 << 18, np.uint32)            # tiles of exactly 2^32: everything far below SAT
    assert sr.defined(sr.exclusive(y)).all()


@pytest.mark.parametrize("t", [0, 1, M32 - 2, M32 - 1, M32, M32 + 1, sr.SAT - 1, sr.SAT, sr.SAT + 1, 1 << 47, (1 << 48) + 5])
def test_total_contract_and_refusal(t):
    tag = 0xBEEF << 48
    want = min(t, sr.SAT)
    assert sr.total(t) == want
    assert sr.total_ok(tag | want, t, tag=tag) and sr.total_ok(want, t, tagged=False)
    assert not sr.total_ok(want, t, tag=tag ^ (1 << 48))
    if 0 < t < sr.SAT:
        assert not sr.total_ok(tag | (t - 1), t, tag=tag)
    if M32 <= t < sr.SAT:
        assert not sr.total_ok(tag | (t % M32), t, tag=tag)   # the 32-bit tile sum's answer
    if t >= sr.SAT:
        assert not sr.total_ok(tag | (t % M32), t, tag=tag)
        # popcounts / bytes: anything from SAT up to the true total (below the tag bits)
        assert sr.total_ok(tag | sr.SAT, t, "popcount", tag=tag)
        assert sr.total_ok(tag | min(t, sr.VALUE_MASK), t, "bytes", tag=tag)
    # every caller's refusal fires exactly when the true total reaches 2^32 - 1, tag or no tag
    assert sr.refused(tag | want) == (t >= M32 - 1) == sr.refused(want)


def brute_sel(x):
    out, acc = {}, 0
    for i, w in enumerate(x):
        v = bin(int(w)).count("1")
        for c in range(acc, acc + v):
            if c % 1024 == 0:
                out[c // 1024] = i
        acc += v
    return [out[c] for c in range(len(out))], acc


@pytest.mark.parametrize("seed,kind", [(0, "random"), (1, "ones"), (2, "sparse"), (3, "zeros")])
def test_sel(seed, kind):
    rng = np.random.default_rng(seed)
    n = 3000
    x = {"random": rng.integers(0, M32, n, dtype=np.uint64).astype(np.uint32), "ones": np.full(n, 0xFFFFFFFF, np.uint32),
         "sparse": np.where(rng.random(n) < 0.05, rng.integers(0, M32, n, dtype=np.uint64), 0).astype(np.uint32),
         "zeros": np.zeros(n, np.uint32)}[kind]
    want, tot = brute_sel(x)
    got = sr.sel(x)
    assert len(got) == (tot + 1023) // 1024 == len(want)
    assert [int(v) for v in got] == want


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33])
def test_group16(n):
    x = np.arange(n, dtype=np.uint32) * 3 + 1
    out = sr.outputs(sr.exclusive(x))
    g = sr.group16(out)
    assert len(g) == n // 16 + 1
    assert [int(v) for v in g] == [int(out[16 * i]) for i in range(n // 16 + 1)]


def test_tiles_and_modes():
    assert sr.ntiles(0) == 1 and sr.ntiles(sr.TILE - 1) == 1 and sr.ntiles(sr.TILE) == 2
    last_gen = sr.GEN_TILES * sr.TILE - 1
    assert sr.gen_mode(last_gen) and not sr.gen_mode(last_gen + 1)
