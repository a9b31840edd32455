/*
 * near_sanitize.c -- the proximity queries' host definition (csrc/near_host.c, with csrc/layers_host.c's list rule, csrc/cast_host.c's
 * argument check and csrc/scene_prep.c) as a stand-alone host program for a sanitizer build:
 *
 *   C=example_gui_opencl_raytracer_amd/csrc
 *   gcc -O1 -g -std=c99 -D_DEFAULT_SOURCE -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I $C \
 *       tools/near_sanitize.c $C/near_host.c $C/layers_host.c $C/cast_host.c $C/projection_host.c $C/host_camera.c $C/scene_prep.c -lm -o near_sanitize
 *   ./near_sanitize
 *
 * It makes its own scene (37 spheres, some glass, one of negative radius, two coincident; 2 planes; 3 lights) and 257 probes from a fixed
 * generator -- points around and inside the spheres, reaches 0, positive, negative, +inf and NaN, a NaN and an infinite coordinate, a point
 * at a centre -- as heap blocks of exactly the sizes the calls are entitled to (so that a read or a write beyond them is the address
 * sanitizer's to report), and runs all 14 flag words that name a kind, with and without ignore words, with n probes and with one: nearest,
 * within, and K = 1..8.  Held to: within == 0 implies the miss record and an empty list; layer 0 == the nearest query wherever that is finite;
 * K is a prefix of K + 1; a listed id lies inside its array.  The refusals are called with output blocks of ONE byte, which they must not
 * touch.  Prints "near_sanitize: N calls, 0 failures"; exit status 1 on a failed check (a sanitizer report aborts).
 * Host code only: nothing here touches a GPU.
 */
#include "near_host.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { NS = 37, NP = 2, NL = 3, N = 257 };
static int failures = 0, calls = 0;
static uint32_t state = 0x2545F491u;
static float rnd(void) { state = state * 1664525u + 1013904223u; return (float)(state >> 8) / 16777216.0f; }      /* [0, 1) */

#define CHECK(c) do { if (!(c)) { failures++; fprintf(stderr, "near_sanitize: line %d: %s\n", __LINE__, #c); } } while (0)

static int id_ok(uint32_t id) {
    const uint32_t kind = id >> 30, index = id & 0x3FFFFFFFu;
    return id == CLW_ID_NONE || (kind == 0u && index < NS) || (kind == 1u && index < NP) || (kind == 2u && index < NL);
}

int main(void) {
    uint8_t* sp = (uint8_t*)calloc(NS, 96);
    uint8_t* pl = (uint8_t*)calloc(NP, 96);
    uint8_t* li = (uint8_t*)calloc(NL, 48);
    clw_probe* pr = (clw_probe*)malloc(N * sizeof(clw_probe));
    uint32_t* ign = (uint32_t*)malloc(N * 4);
    for (int i = 0; i < NS; i++) {
        float c[4] = {rnd() * 8.0f - 4.0f, rnd() * 4.0f, rnd() * 8.0f - 4.0f, 0.2f + rnd()};
        if (i == 5) c[3] = -c[3];
        if (i == 9) memcpy(c, sp + 96 * 8, 12);      /* coincides with sphere 8 */
        memcpy(sp + 96 * i, c, 12);
        memcpy(sp + 96 * i + 16, &c[3], 4);
        const uint32_t glass = (i % 7) == 3;
        memcpy(sp + 96 * i + 64, &glass, 4);
    }
    const float planes[NP][6] = {{0, 1, 0, 0, 0, 0}, {0.5f, 2, 0.25f, 1, -1, 2}};
    for (int i = 0; i < NP; i++) { memcpy(pl + 96 * i, planes[i], 12); memcpy(pl + 96 * i + 16, planes[i] + 3, 12); }
    for (int i = 0; i < NL; i++) { const float l[5] = {rnd() * 6.0f - 3.0f, 5.0f, rnd() * 6.0f - 3.0f, 0, 0.3f}; memcpy(li + 48 * i, l, 12); memcpy(li + 48 * i + 16, &l[4], 4); }
    for (int k = 0; k < N; k++) {
        const int i = k % NS;
        float c[3], r;
        memcpy(c, sp + 96 * i, 12);
        memcpy(&r, sp + 96 * i + 16, 4);
        const float off = (k % 3 == 0 ? rnd() * 0.9f : 1.0f + rnd() * 2.0f) * fabsf(r);      /* inside, or up to two radii off */
        pr[k].point[0] = c[0] + off; pr[k].point[1] = c[1] - 0.5f * off; pr[k].point[2] = c[2] + 0.25f * off;
        const float reaches[6] = {0.0f, 0.5f, 2.0f, -0.25f, INFINITY, 1.0f};
        pr[k].reach = reaches[k % 6];
        if (k % 41 == 7) pr[k].point[k % 3] = NAN;
        if (k % 41 == 11) pr[k].reach = NAN;
        if (k % 41 == 13) pr[k].point[k % 3] = (k & 1) ? INFINITY : -INFINITY;
        if (k % 41 == 17) memcpy(pr[k].point, c, 12);
        ign[k] = k % 4 == 1 ? (uint32_t)i : (k % 4 == 2 ? (1u << 30) : CLW_ID_NONE);
    }
    for (uint32_t flags = 1; flags < 16; flags++) {
        if (!(flags & CLW_CAST_KINDS)) continue;
        for (int with_ignore = 0; with_ignore < 2; with_ignore++)
            for (uint32_t n = N; n >= 1; n = n == 1 ? 0 : 1) {
                const uint32_t* ig = with_ignore ? ign : NULL;
                clw_hit* hits = (clw_hit*)malloc(n * sizeof(clw_hit));
                uint8_t* within = (uint8_t*)malloc(n);
                float* prev_d = NULL; uint32_t* prev_id = NULL;
                CHECK(clw_host_nearest_surface(pr, ig, n, flags, sp, NS, pl, NP, li, NL, hits) == 1);
                CHECK(clw_host_within_reach(pr, ig, n, flags, sp, NS, pl, NP, li, NL, within) == 1);
                calls += 2;
                for (uint32_t K = 1; K <= 8; K++) {
                    float* d = (float*)malloc((size_t)K * n * 4);
                    uint32_t* id = (uint32_t*)malloc((size_t)K * n * 4);
                    CHECK(clw_host_near_surfaces(pr, ig, n, flags, sp, NS, pl, NP, li, NL, K, d, id) == 1);
                    calls++;
                    for (uint32_t k = 0; k < n; k++) {
                        for (uint32_t j = 0; j < K; j++) CHECK(id_ok(id[j * n + k]) && (id[j * n + k] == CLW_ID_NONE) == (d[j * n + k] == INFINITY));
                        if (!within[k]) CHECK(hits[k].id == CLW_ID_NONE && hits[k].t == INFINITY && id[k] == CLW_ID_NONE);
                        if (hits[k].t < INFINITY) CHECK(hits[k].id == id[k] && memcmp(&hits[k].t, &d[k], 4) == 0 && within[k] == 1);
                        CHECK(id_ok(hits[k].id) && (!with_ignore || hits[k].id == CLW_ID_NONE || hits[k].id != ign[k]));
                    }
                    if (prev_d) CHECK(memcmp(prev_d, d, (size_t)(K - 1) * n * 4) == 0 && memcmp(prev_id, id, (size_t)(K - 1) * n * 4) == 0);
                    free(prev_d); free(prev_id);
                    prev_d = d; prev_id = id;
                }
                free(prev_d); free(prev_id); free(hits); free(within);
            }
    }
    /* refusals: one byte of output, untouched */
    uint8_t* one = (uint8_t*)malloc(1);
    uint8_t* two = (uint8_t*)malloc(1);
    *one = *two = 0xA5;
    CHECK(clw_host_nearest_surface(pr, NULL, 0, 3, sp, NS, pl, NP, li, NL, (clw_hit*)one) == 0);
    CHECK(clw_host_nearest_surface(pr, NULL, N, 0, sp, NS, pl, NP, li, NL, (clw_hit*)one) == 0);
    CHECK(clw_host_nearest_surface(pr, NULL, N, 16 | 3, sp, NS, pl, NP, li, NL, (clw_hit*)one) == 0);
    CHECK(clw_host_nearest_surface(NULL, NULL, N, 3, sp, NS, pl, NP, li, NL, (clw_hit*)one) == 0);
    CHECK(clw_host_nearest_surface(pr, NULL, N, 3, NULL, NS, pl, NP, li, NL, (clw_hit*)one) == 0);
    CHECK(clw_host_nearest_surface(pr, NULL, N, 3, sp, NS, pl, NP, li, NL, NULL) == 0);
    CHECK(clw_host_within_reach(pr, NULL, 1u << 30, 3, sp, NS, pl, NP, li, NL, one) == 0);
    CHECK(clw_host_within_reach(pr, NULL, N, 8, sp, NS, pl, NP, li, NL, one) == 0);
    CHECK(clw_host_near_surfaces(pr, NULL, N, 3, sp, NS, pl, NP, li, NL, 0, (float*)one, (uint32_t*)two) == 0);
    CHECK(clw_host_near_surfaces(pr, NULL, N, 3, sp, NS, pl, NP, li, NL, 9, (float*)one, (uint32_t*)two) == 0);
    CHECK(clw_host_near_surfaces(pr, NULL, N, 3, sp, NS, pl, NP, li, NL, 4, NULL, (uint32_t*)two) == 0);
    CHECK(clw_host_near_surfaces(pr, NULL, N, 3, sp, NS, pl, NP, li, NL, 4, (float*)one, NULL) == 0);
    CHECK(*one == 0xA5 && *two == 0xA5);
    free(one); free(two); free(sp); free(pl); free(li); free(pr); free(ign);
    printf("near_sanitize: %d calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
