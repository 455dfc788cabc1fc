"""Numpy restatement of the device-wide exclusive prefix scan (vx_kernels.hip: launch_scan_u32, launch_scan_u8; vx_scan_u32), for the tests.

f(x) = the element itself (mode "values", uint32), its popcount ("popcount", uint32 words) or the byte ("bytes", uint8).  The exact
exclusive prefix P[i] = sum_{j < i} f(x[j]) for i in 0..n, in uint64 (n + 1 entries; P[n] = T, the true total).

- out[i] = P[i] mod 2^32, for every 16384-element tile (the single-pass tile) whose exclusive prefix P[16384 t] is below SAT.  Past that
  the total has saturated and every caller refuses the scan: the outputs are unspecified.
- the total: T while T < SAT; from there on SAT for values (and on the three-pass path); for popcounts and bytes at least SAT and below
  2^48.  The single-pass paths OR total_tag (bits 48..63) into it.  So `total & (2^48 - 1) >= 0xFFFFFFFF` (every caller's refusal) holds
  exactly when T >= 2^32 - 1.
- sel[c] (popcounts only: values of at most 1024) = the index i of the element whose range [P[i], P[i] + f(x[i])) holds c * 1024, for
  every c with c * 1024 < T.
- group16[i] = out[16 i] for i in 0..n // 16.
"""
import numpy as np

SAT = (1 << 40) - 1          # kScanTotalSat
VALUE_MASK = (1 << 48) - 1   # kMailValue: the bits below a total's tag
TILE = 16384                 # single-pass tile (1024 threads x 16 elements)
GEN_TILES = 512              # kScanGenTiles: larger single-pass scans run in ticket mode
REFUSE = 0xFFFFFFFF          # every caller: `total >= 0xFFFFFFFF` is a capacity error


def elements(x, mode):
    """f(x) as uint64."""
    if mode == "values":
        return np.asarray(x, dtype=np.uint32).astype(np.uint64)
    if mode == "popcount":
        b = np.asarray(x, dtype=np.uint32).view(np.uint8)
        return np.unpackbits(b).reshape(-1, 32).sum(1, dtype=np.uint64) if b.size else np.zeros(0, np.uint64)
    if mode == "bytes":
        return np.asarray(x, dtype=np.uint8).astype(np.uint64)
    raise ValueError(mode)


def exclusive(x, mode="values"):
    """P[0..n] in uint64 (exact: n < 2^32 elements of at most 2^32 - 1)."""
    v = elements(x, mode)
    p = np.zeros(v.size + 1, np.uint64)
    np.cumsum(v, out=p[1:])
    return p


def outputs(p):
    """out[0..n] = P mod 2^32."""
    return (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def defined(p):
    """which of out[0..n] the contract specifies: the entries of tiles whose exclusive prefix is below SAT."""
    starts = p[np.arange(0, p.size, TILE)]
    return np.repeat(starts < np.uint64(SAT), TILE)[: p.size]


def total(true_total):
    """the total of a values scan (and of the three-pass path) without its tag."""
    return min(int(true_total), SAT)


def total_ok(word, true_total, mode="values", tag=0, tagged=True):
    """whether a total word meets the contract."""
    t = int(true_total)
    if tagged:
        if word & ~VALUE_MASK != tag:
            return False
        word &= VALUE_MASK
    elif word >> 48:
        return False
    if t < SAT:
        return word == t
    return word == SAT if mode == "values" or not tagged else SAT <= word <= min(t, VALUE_MASK)


def refused(word):
    """every caller's capacity check on a total word."""
    return (word & VALUE_MASK) >= REFUSE


def sel(x, p=None):
    """sel[0..ceil(T / 1024)) for a popcount scan."""
    v = elements(x, "popcount")
    if p is None:
        p = exclusive(x, "popcount")
    incl = p[1:]
    marks = np.arange(0, int(p[-1]), 1024, dtype=np.uint64)
    return np.searchsorted(incl, marks, side="right").astype(np.uint32) if v.size else np.zeros(0, np.uint32)


def group16(out):
    """group16[0..n // 16] from out[0..n]."""
    return np.ascontiguousarray(out[::16])


def ntiles(n):
    """single-pass tiles of a scan of n elements (n + 1 outputs)."""
    return (n + 1 + TILE - 1) // TILE


def gen_mode(n):
    """whether a generation-numbered single-pass scan of n elements runs in generation mode (else ticket mode)."""
    return ntiles(n) <= GEN_TILES
