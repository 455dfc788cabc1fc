"""The device-wide exclusive prefix scan (vx_kernels.hip) against tests/scan_ref.py, through the vx_scan_u32 test aid.

Every case runs on the three paths -- single-pass generation mode, single-pass ticket mode, three passes -- which must agree with each
other and with the reference: every output entry the contract specifies, the canaries behind out[n], sel and group16, the 64-bit total
(exact below 2^40 - 1, saturated above, tag bits intact) and the scratch block's state after every scan.
"""
import numpy as np
import pytest

import scan_ref as sr

pytestmark = pytest.mark.gpu

PATHS = ("gen", "ticket", "three")
TAG = 0x5A3C << 48
CANARY = 0xA5A5A5A5
LAST_GEN = sr.GEN_TILES * sr.TILE - 1        # the last size a generation-numbered scan runs in generation mode


def expect_path(path, n, in_offset=0, out_offset=0, mode="values"):
    if path == "three" or (mode != "bytes" and (in_offset or out_offset)):
        return "three"
    if path == "gen" and not sr.gen_mode(n):
        return "ticket"
    return path


def check(r, x, mode, path, what, tag=TAG, sel_cap=0, group16_cap=0):
    """one scan's result against the reference"""
    n = len(x)
    p = sr.exclusive(x, mode)
    t = int(p[-1])
    want = sr.outputs(p)
    d = sr.defined(p)
    got = r["out"]
    assert len(got) == n + 1
    bad = np.flatnonzero((got != want) & d)
    assert bad.size == 0, "%s: %d wrong outputs, first at %d: %d != %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert (r["canary"] == CANARY).all(), "%s: written past out[n]" % what
    tagged = r["taken"] != "three"
    assert sr.total_ok(r["total"], t, mode, tag=tag, tagged=tagged), "%s: total %#x, true %#x" % (what, r["total"], t)
    assert sr.refused(r["total"]) == (t >= sr.REFUSE), what
    assert r["clean"], "%s: the scratch block is not in the state the next scan relies on" % what
    if group16_cap:
        g = r["group16"]
        if r["taken"] == "three":
            assert (g == CANARY).all(), what
        else:
            k = n // 16 + 1
            gw, gd = sr.group16(want), sr.group16(d)
            assert np.array_equal(g[:k][gd], gw[gd]) and (g[k:] == CANARY).all(), "%s: group16" % what
    if sel_cap:
        s = r["sel"]
        if r["taken"] == "three":
            assert (s == CANARY).all(), what
        else:
            ws = sr.sel(x, p)
            assert np.array_equal(s[:len(ws)], ws) and (s[len(ws):] == CANARY).all(), "%s: sel" % what
    return got


def run_all(gpu, x, mode="values", what="", **kw):
    """the same input on the three paths; they agree on every specified output"""
    outs = []
    for path in PATHS:
        r = gpu.scan_u32([x], mode=mode, paths=path, total_tag=TAG, **kw)[0]
        assert r["taken"] == expect_path(path, len(x), kw.get("in_offset", 0), kw.get("out_offset", 0), mode), (what, path, r["taken"])
        outs.append((path, check(r, x, mode, path, "%s [%s]" % (what, path), sel_cap=kw.get("sel_cap", 0), group16_cap=kw.get("group16_cap", 0))))
    return outs


SIZES = [0, 1, 2, 15, 16, 17, 2047, 2048, 2049, sr.TILE - 1, sr.TILE, sr.TILE + 1]


def values(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "small":
        return rng.integers(0, 1000, n, dtype=np.uint32)
    if kind == "full":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "huge_last":
        x = rng.integers(0, 1000, n, dtype=np.uint32)
        if n:
            x[-1] = 0xFFFFFFFF
        return x
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["zeros", "ones", "small", "full", "huge_last"])
def test_scan_sizes(gpu, kind):
    rng = np.random.default_rng(["zeros", "ones", "small", "full", "huge_last"].index(kind) + 11)
    for n in SIZES:
        x = values(kind, n, rng)
        run_all(gpu, x, what="%s n=%d" % (kind, n), group16_cap=n // 16 + 1 + 16)


@pytest.mark.parametrize("n", [LAST_GEN, LAST_GEN + 1])
def test_scan_generation_ticket_boundary(gpu, n):
    """512 tiles of 16384 minus one element: the last generation-mode scan; one more: ticket mode"""
    rng = np.random.default_rng(n)
    run_all(gpu, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), what="n=%d" % n, group16_cap=n // 16 + 1 + 16)
    run_all(gpu, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), mode="popcount", what="popcount n=%d" % n,
            sel_cap=(32 * n) // 1024 + 16, group16_cap=n // 16 + 1 + 16)


def test_scan_many_tiles_ticket(gpu):
    """one ticket-mode scan of 2500 tiles (a look-back chain far longer than the 64-word window)"""
    n = 2500 * sr.TILE - 7
    x = np.random.default_rng(9).integers(0, 1 << 20, n, dtype=np.uint32)
    run_all(gpu, x, what="2500 tiles")


def test_scan_pairs_around_2_31(gpu):
    for pair in [((1 << 31) - 1, 1 << 31), (1 << 31, 1 << 31), (1 << 31, (1 << 31) + 1), (0xFFFFFFFF, 1)]:
        run_all(gpu, np.array(pair, np.uint32), what="pair %r" % (pair,))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_scan_tile_sum_2_32(gpu, delta):
    """one tile whose values add up to 2^32 + delta (the single-pass tile total used to be 32-bit: 2^32 read as 0), alone and as
    the middle one of three tiles"""
    tile = np.full(sr.TILE, 1 << 18, np.uint32)            # 16384 * 2^18 = 2^32
    tile[-1] = np.uint32((1 << 18) + delta)
    assert int(tile.astype(np.uint64).sum()) == (1 << 32) + delta
    run_all(gpu, tile, what="one tile, 2^32%+d" % delta)
    rng = np.random.default_rng(delta + 5)
    x = np.concatenate([rng.integers(0, 1 << 10, sr.TILE, dtype=np.uint32), tile, rng.integers(0, 1 << 10, sr.TILE + 3, dtype=np.uint32)])
    run_all(gpu, x, what="three tiles, 2^32%+d" % delta)


def test_scan_saturation_and_tag(gpu):
    """all 0xFFFFFFFF: one tile alone sums to ~2^46 (past the 40-bit generation-mode field), five pass 2^48 (the tag bits): the total
    saturates at 2^40 - 1 below the tag on every path, in generation mode and in ticket mode"""
    for n in (sr.TILE - 1, 5 * sr.TILE + 3):
        x = np.full(n, 0xFFFFFFFF, np.uint32)
        outs = run_all(gpu, x, what="all ones n=%d" % n)
        for _, o in outs:
            assert np.array_equal(o[: sr.TILE], outs[0][1][: sr.TILE])


def test_scan_popcount(gpu):
    rng = np.random.default_rng(3)
    for n in (0, 1, 17, 2049, sr.TILE + 1, 5 * sr.TILE - 1):
        for kind, x in (("random", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)), ("ones", np.full(n, 0xFFFFFFFF, np.uint32)),
                        ("sparse", np.where(rng.random(n) < 0.02, rng.integers(0, 1 << 32, n, dtype=np.uint64), 0).astype(np.uint32))):
            run_all(gpu, x, mode="popcount", what="popcount %s n=%d" % (kind, n), sel_cap=(32 * n) // 1024 + 16, group16_cap=n // 16 + 1 + 16)


def test_scan_bytes(gpu):
    """bytes: n not a multiple of 16, aligned and unaligned starts (the byte scan has no three-pass path; unaligned tiles go element-wise)"""
    rng = np.random.default_rng(4)
    for n in (0, 1, 15, 17, 4099, sr.TILE + 5, 3 * sr.TILE - 1):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        for path in ("gen", "ticket"):
            for ioff, ooff in ((0, 0), (3, 0), (0, 1), (5, 3)):
                r = gpu.scan_u32([x], mode="bytes", paths=path, in_offset=ioff, out_offset=ooff, total_tag=TAG)[0]
                assert r["taken"] == path
                check(r, x, "bytes", path, "bytes n=%d %s offsets %d/%d" % (n, path, ioff, ooff))
        x = np.full(n, 255, np.uint8)
        check(gpu.scan_u32([x], mode="bytes", paths="gen", total_tag=TAG)[0], x, "bytes", "gen", "bytes 255 n=%d" % n)


def test_scan_unaligned_falls_back(gpu):
    """misaligned in / out take the three-pass path whatever the call asks, with the same results"""
    rng = np.random.default_rng(6)
    for n in (17, sr.TILE + 1):
        x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        for ioff, ooff in ((1, 0), (0, 2), (3, 1)):
            run_all(gpu, x, what="offsets %d/%d n=%d" % (ioff, ooff, n), in_offset=ioff, out_offset=ooff)


def test_scan_sequence_one_scratch_block(gpu):
    """growing and shrinking sizes, generation, ticket and three-pass scans interleaved on one scratch block: every scan checked"""
    rng = np.random.default_rng(7)
    sizes = [1, 20000, 16383, 300000, 17, 0, 2049, LAST_GEN + 1, 5, 100000, 16385, 3, 70000]
    paths = ["gen", "gen", "ticket", "gen", "three", "gen", "ticket", "gen", "gen", "three", "gen", "ticket", "gen"]
    for mode in ("values", "popcount"):
        xs = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in sizes]
        rs = gpu.scan_u32(xs, mode=mode, paths=paths, total_tag=TAG, group16_cap=max(sizes) // 16 + 17)
        for k, (x, p, r) in enumerate(zip(xs, paths, rs)):
            assert r["taken"] == expect_path(p, len(x)), (k, p, r["taken"])
            check(r, x, mode, p, "%s scan %d (%s, n=%d)" % (mode, k, p, len(x)), group16_cap=max(sizes) // 16 + 17)


def test_scan_generation_wrap(gpu):
    """a run across the wrap of the generation counter at 2^22 (the block is cleared and numbering restarts at 1), with words of
    larger scans of the old numbering left behind"""
    rng = np.random.default_rng(8)
    sizes = [200000, 3 * sr.TILE, 17, 150000, 40000, 1, 250000, 16384]
    paths = ["gen"] * len(sizes)
    paths[4] = "ticket"
    xs = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in sizes]
    rs = gpu.scan_u32(xs, paths=paths, total_tag=TAG, gen_start=(1 << 22) - 4)
    for k, (x, p, r) in enumerate(zip(xs, paths, rs)):
        check(r, x, "values", p, "scan %d across the wrap (n=%d)" % (k, len(x)))
    rs = gpu.scan_u32([xs[0], xs[1]], paths="gen", total_tag=TAG, gen_start=(1 << 22) - 1)   # the very first scan wraps
    for k, r in enumerate(rs):
        check(r, xs[k], "values", "gen", "wrap at the first scan %d" % k)


def test_scan_auto_is_generation_mode(gpu):
    """the library's own scans (the auto path): two consecutive scans of 40000 values on one scratch block both run in generation mode,
    the second gives the right total and leaves the block in the state the next scan relies on"""
    x = np.arange(40000, dtype=np.uint32)
    r = gpu.scan_u32([x, x], paths="auto")
    got = "%s %s %s %s" % (r[0]["taken"], r[1]["taken"], int(r[1]["out"][-1]) == int(x.astype(np.uint64).sum()), r[1]["clean"])
    assert got == "gen gen True True", got
