/* nearest_ref.c -- test helper: the feature transform of a uint8 target mask [Z][Y][X] in plain C, for fields too large for the numpy
 * restatement (tests/nearest_ref.py).  out[i(c)] = the cell index x + X*(y + Y*z) of the target nearest to c, the smallest index among
 * equally near ones; 0xFFFFFFFF where no target exists.  Along x the nearer of the last and the next target of the row, the left one on a
 * tie; along y and z the linear lower envelope of the parabolas (i - j)^2 + g(j) per column (Meijster et al.), each entry carrying the target
 * its g belongs to: a parabola is dropped only when the newcomer is strictly better where the parabola starts, and a newcomer starts where it
 * is strictly better, so the smaller j keeps every tie.  64-bit integers throughout.  Returns 0, or -1 when a work array cannot be allocated. */
#include <stdint.h>
#include <stdlib.h>

#define INF 0xFFFFFFFFull

static uint64_t f(int64_t x, int64_t s, uint64_t g) { return (uint64_t)((x - s) * (x - s)) + g; }

/* the envelope of g[0..n): win[u] = the j whose parabola is lowest at u (the smallest such j), -1 when every g is INF */
static void envelope(const uint64_t* g, int64_t n, int64_t* s, int64_t* t, int64_t* win)
{
    int64_t q = -1;
    for (int64_t u = 0; u < n; ++u) {
        if (g[u] == INF) continue;
        while (q >= 0 && f(t[q], s[q], g[s[q]]) > f(t[q], u, g[u])) --q;
        if (q < 0) { q = 0; s[0] = u; t[0] = 0; continue; }
        const int64_t num = u * u - s[q] * s[q] + (int64_t)g[u] - (int64_t)g[s[q]];
        const int64_t den = 2 * (u - s[q]);
        const int64_t w = (num >= 0 ? num / den : -((-num + den - 1) / den)) + 1;
        if (w < n) { ++q; s[q] = u; t[q] = w; }
    }
    for (int64_t u = n - 1; u >= 0; --u) {
        win[u] = q < 0 ? -1 : s[q];
        if (q >= 0 && u == t[q]) --q;
    }
}

int nearest(const uint8_t* target, uint32_t* out, uint32_t X, uint32_t Y, uint32_t Z)
{
    const uint64_t N = (uint64_t)X * Y * Z;
    const uint64_t nmax = Y > Z ? Y : Z;
    int32_t* fx = malloc(N * sizeof(int32_t)); /* x' of the nearest target within the row, then within the plane; -1: none */
    int32_t* fy = malloc(N * sizeof(int32_t)); /* y' of the nearest target within the plane */
    uint64_t* g = malloc(nmax * sizeof(uint64_t));
    int64_t* s = malloc(nmax * sizeof(int64_t));
    int64_t* t = malloc(nmax * sizeof(int64_t));
    int64_t* win = malloc(nmax * sizeof(int64_t));
    int32_t* cx = malloc(nmax * sizeof(int32_t));
    int32_t* cy = malloc(nmax * sizeof(int32_t));
    int rc = -1;
    if (!fx || !fy || !g || !s || !t || !win || !cx || !cy) goto done;
    for (uint64_t r = 0; r < (uint64_t)Y * Z; ++r) {
        const uint8_t* m = target + r * X;
        int32_t* o = fx + r * X;
        int64_t last = -1;
        for (int64_t x = 0; x < X; ++x) {
            if (m[x]) last = x;
            o[x] = (int32_t)last;
        }
        last = -1;
        for (int64_t x = (int64_t)X - 1; x >= 0; --x) {
            if (m[x]) last = x;
            if (last >= 0 && (o[x] < 0 || last - x < x - o[x])) o[x] = (int32_t)last; /* the right one only when strictly nearer */
        }
    }
    for (uint64_t z = 0; z < Z; ++z)
        for (uint64_t x = 0; x < X; ++x) {
            const uint64_t base = z * X * Y + x;
            for (uint64_t u = 0; u < Y; ++u) {
                cx[u] = fx[base + u * X];
                g[u] = cx[u] < 0 ? INF : (uint64_t)(((int64_t)x - cx[u]) * ((int64_t)x - cx[u]));
            }
            envelope(g, Y, s, t, win);
            for (uint64_t u = 0; u < Y; ++u) {
                fx[base + u * X] = win[u] < 0 ? -1 : cx[win[u]];
                fy[base + u * X] = (int32_t)win[u];
            }
        }
    for (uint64_t c = 0; c < (uint64_t)X * Y; ++c) {
        const int64_t x = (int64_t)(c % X), y = (int64_t)(c / X);
        for (uint64_t u = 0; u < Z; ++u) {
            cx[u] = fx[c + u * X * Y];
            cy[u] = fy[c + u * X * Y];
            g[u] = cx[u] < 0 ? INF : (uint64_t)((x - cx[u]) * (x - cx[u]) + (y - cy[u]) * (y - cy[u]));
        }
        envelope(g, Z, s, t, win);
        for (uint64_t u = 0; u < Z; ++u)
            out[c + u * X * Y] = win[u] < 0 ? (uint32_t)INF : (uint32_t)((uint64_t)cx[win[u]] + X * ((uint64_t)cy[win[u]] + Y * (uint64_t)win[u]));
    }
    rc = 0;
done:
    free(fx);
    free(fy);
    free(g);
    free(s);
    free(t);
    free(win);
    free(cx);
    free(cy);
    return rc;
}
