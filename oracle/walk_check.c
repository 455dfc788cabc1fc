/*
 * walk_check.c -- TEST INFRASTRUCTURE: a stand-alone driver of vx_walk.c, so that the CPU walker can run under the host sanitizers
 * as a program of its own (no interpreter around it, nothing to preload):
 *
 *     gcc -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -ffp-contract=off \
 *         walk_check.c vx_walk.c -lm -lpthread -o walk_check  &&  ./walk_check case.bin
 *
 * case.bin (little endian; tests/ray_nonfinite.py write_walk_case):
 *     uint64 dim[3]; float vs; float org[3]; uint64 nwords; uint64 nrays; uint64 nfinite;
 *     uint32 words[nwords]; float rays[nrays][6]; float t_ref[nfinite]; uint64 idx_ref[nfinite];
 * The first nfinite rays are finite and must give t_ref / idx_ref bit for bit (the walker still walks); every ray after them has a
 * NaN or +-Inf component and must miss (t = -1, idx = ~0) on [0.001, 10000] and on [0, +inf].  Exit status 0: all of that held.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct walk_grid walk_grid;
walk_grid* vxo_walk_create(const uint32_t* words, const uint64_t dim[3], float vs, const float org[3]);
void vxo_walk_free(walk_grid* g);
void vxo_walk_trace(const walk_grid* g, const float* rays, uint64_t nrays, float tmin, float tmax, int threads, float* t_out, uint64_t* idx_out,
                    uint64_t* stats4);

static int get(void* p, size_t size, size_t n, FILE* fh) { return n == 0 || fread(p, size, n, fh) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: walk_check case.bin\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    uint64_t dim[3], n[3];
    float vs, org[3];
    if (!get(dim, 8, 3, fh) || !get(&vs, 4, 1, fh) || !get(org, 4, 3, fh) || !get(n, 8, 3, fh)) { fprintf(stderr, "short header\n"); return 2; }
    const uint64_t nwords = n[0], nrays = n[1], nfinite = n[2];
    if (nfinite > nrays || nwords < (dim[0] * dim[1] * dim[2] + 31) / 32) { fprintf(stderr, "bad header\n"); return 2; }
    uint32_t* words = (uint32_t*)calloc(nwords + 1, 4);
    float* rays = (float*)calloc(6 * nrays + 1, 4);
    float* t_ref = (float*)calloc(nfinite + 1, 4);
    uint64_t* idx_ref = (uint64_t*)calloc(nfinite + 1, 8);
    float* t = (float*)calloc(nrays + 1, 4);
    uint64_t* idx = (uint64_t*)calloc(nrays + 1, 8);
    if (!get(words, 4, nwords, fh) || !get(rays, 4, 6 * nrays, fh) || !get(t_ref, 4, nfinite, fh) || !get(idx_ref, 8, nfinite, fh)) {
        fprintf(stderr, "short file\n");
        return 2;
    }
    fclose(fh);
    walk_grid* g = vxo_walk_create(words, dim, vs, org);
    uint64_t bad = 0, finite_hits = 0;
    const float iv[2][2] = {{0.001f, 10000.0f}, {0.0f, INFINITY}};
    for (int k = 0; k < 2; ++k) {
        for (int threads = 1; threads <= 4; threads += 3) {
            memset(t, 0, (size_t)nrays * 4);
            memset(idx, 0, (size_t)nrays * 8);
            vxo_walk_trace(g, rays, nrays, iv[k][0], iv[k][1], threads, t, idx, NULL);
            for (uint64_t r = 0; r < nrays; ++r) {
                int ok;
                if (r < nfinite && k == 0) {
                    ok = memcmp(&t[r], &t_ref[r], 4) == 0 && idx[r] == idx_ref[r];
                    finite_hits += t[r] > 0.0f;
                } else if (r < nfinite) {
                    ok = 1;  /* (the reference in the file is the one of the default interval) */
                } else {
                    ok = t[r] == -1.0f && idx[r] == ~0ull;
                }
                if (!ok && bad++ < 10)
                    fprintf(stderr, "ray %llu [%g, %g] threads %d: t %a idx %llx  (%a %a %a  %a %a %a)\n", (unsigned long long)r, iv[k][0], iv[k][1], threads,
                            t[r], (unsigned long long)idx[r], rays[6 * r], rays[6 * r + 1], rays[6 * r + 2], rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]);
            }
        }
    }
    vxo_walk_free(g);
    free(words); free(rays); free(t_ref); free(idx_ref); free(t); free(idx);
    printf("walk_check: %llu rays (%llu finite, %llu of them hit), %llu wrong\n", (unsigned long long)nrays, (unsigned long long)nfinite,
           (unsigned long long)(finite_hits / 2), (unsigned long long)bad);
    return bad ? 1 : 0;
}
