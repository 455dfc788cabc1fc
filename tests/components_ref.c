/* components_ref.c -- test helper: connected-component labels of a uint8 mask [Z][Y][X] in plain C, for grids too large for the numpy
 * restatement (tests/components_ref.py).  Sequential union-find over the occupied cells in ascending index: every cell is joined with its
 * occupied backward neighbours (3 offsets for 6-connectivity, 13 for 26), the larger root linked to the smaller, so every root is the
 * smallest cell of its set.  Then one ascending pass numbers the roots 1, 2, ... and gives every other cell its root's label.
 * Out: uint32 labels, 0 for empty cells; returns K, or -1 when the work array cannot be allocated. */
#include <stdint.h>
#include <stdlib.h>

static uint32_t find(uint32_t* p, uint32_t a)
{
    while (p[a] != a) {
        p[a] = p[p[a]];
        a = p[a];
    }
    return a;
}

static void unite(uint32_t* p, uint32_t a, uint32_t b)
{
    a = find(p, a);
    b = find(p, b);
    if (a < b) p[b] = a;
    else if (b < a) p[a] = b;
}

int64_t label(const uint8_t* m, uint32_t* out, uint32_t X, uint32_t Y, uint32_t Z, int connectivity)
{
    const uint64_t n = (uint64_t)X * Y * Z;
    uint32_t* p = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    if (!p) return -1;
    uint64_t i = 0;
    for (uint32_t z = 0; z < Z; ++z)
        for (uint32_t y = 0; y < Y; ++y)
            for (uint32_t x = 0; x < X; ++x, ++i) {
                p[i] = (uint32_t)i;
                if (!m[i]) continue;
                for (int dz = -1; dz <= 0; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;  /* backward offsets only */
                            if (connectivity == 6 && abs(dx) + abs(dy) + abs(dz) != 1) continue;
                            const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
                            if (nx < 0 || ny < 0 || nz < 0 || nx >= X || ny >= Y) continue;
                            const uint64_t j = (uint64_t)nx + (uint64_t)X * ((uint64_t)ny + (uint64_t)Y * (uint64_t)nz);
                            if (m[j]) unite(p, (uint32_t)i, (uint32_t)j);
                        }
            }
    int64_t k = 0;
    for (i = 0; i < n; ++i) {
        if (!m[i]) { out[i] = 0; continue; }
        const uint32_t r = find(p, (uint32_t)i);
        out[i] = r == i ? (uint32_t)++k : out[r];  /* r < i: its label is already written */
    }
    free(p);
    return k;
}
