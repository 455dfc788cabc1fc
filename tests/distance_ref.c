/* distance_ref.c -- test helper: the exact squared Euclidean distance transform of a uint8 target mask [Z][Y][X] in plain C, for fields
 * too large for the numpy restatement (tests/distance_ref.py).  Along x the nearest target of the row (two sweeps), along y and z the
 * linear lower envelope of the parabolas (i - j)^2 + g(j) per column (Meijster et al.), sentinel entries skipped, 64-bit integers
 * throughout.  Out: uint32, 0xFFFFFFFF where no target exists.  Returns 0, or -1 when a work array cannot be allocated. */
#include <stdint.h>
#include <stdlib.h>

#define INF 0xFFFFFFFFull

static uint64_t f(int64_t x, int64_t s, uint64_t g) { return (uint64_t)((x - s) * (x - s)) + g; }

/* one column of n values at a[k * stride], in place; g, s, t: n entries of work space */
static void column(uint32_t* a, uint64_t stride, int64_t n, uint64_t* g, int64_t* s, int64_t* t)
{
    int64_t q = -1;
    for (int64_t u = 0; u < n; ++u) {
        g[u] = a[(uint64_t)u * stride];
        if (g[u] == INF) continue;
        while (q >= 0 && f(t[q], s[q], g[s[q]]) > f(t[q], u, g[u])) --q;
        if (q < 0) { q = 0; s[0] = u; t[0] = 0; continue; }
        const int64_t num = u * u - s[q] * s[q] + (int64_t)g[u] - (int64_t)g[s[q]];
        const int64_t den = 2 * (u - s[q]);
        const int64_t w = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;
        if (w < n) { ++q; s[q] = u; t[q] = w; }
    }
    for (int64_t u = n - 1; u >= 0; --u) {
        a[(uint64_t)u * stride] = q < 0 ? (uint32_t)INF : (uint32_t)f(u, s[q], g[s[q]]);
        if (q >= 0 && u == t[q]) --q;
    }
}

int edt_sq(const uint8_t* target, uint32_t* out, uint32_t X, uint32_t Y, uint32_t Z)
{
    const uint64_t nmax = X > Y ? (X > Z ? X : Z) : (Y > Z ? Y : Z);
    uint64_t* g = malloc(nmax * sizeof(uint64_t));
    int64_t* s = malloc(nmax * sizeof(int64_t));
    int64_t* t = malloc(nmax * sizeof(int64_t));
    if (!g || !s || !t) { free(g); free(s); free(t); return -1; }
    for (uint64_t r = 0; r < (uint64_t)Y * Z; ++r) {
        const uint8_t* m = target + r * X;
        uint32_t* o = out + r * X;
        int64_t last = -1;
        for (int64_t x = 0; x < X; ++x) {
            if (m[x]) last = x;
            o[x] = last < 0 ? (uint32_t)INF : (uint32_t)((x - last) * (x - last));
        }
        last = -1;
        for (int64_t x = (int64_t)X - 1; x >= 0; --x) {
            if (m[x]) last = x;
            if (last >= 0 && (uint64_t)((last - x) * (last - x)) < o[x]) o[x] = (uint32_t)((last - x) * (last - x));
        }
    }
    for (uint64_t z = 0; z < Z; ++z)
        for (uint64_t x = 0; x < X; ++x) column(out + z * X * Y + x, X, Y, g, s, t);
    for (uint64_t c = 0; c < (uint64_t)X * Y; ++c) column(out + c, (uint64_t)X * Y, Z, g, s, t);
    free(g);
    free(s);
    free(t);
    return 0;
}
