/*
 * paths_sanitize.c -- the path queries' definition (csrc/paths_host.c: clw_host_cast_paths) as a stand-alone host program for a sanitizer
 * build:
 *
 *   gcc -O1 -g -std=c99 -ffp-contract=off -D_DEFAULT_SOURCE -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/paths_sanitize.c example_gui_opencl_raytracer_amd/csrc/paths_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/cast_host.c example_gui_opencl_raytracer_amd/csrc/scene_prep.c -lm -o paths_sanitize
 *   ./paths_sanitize CASE.bin ...
 *
 * A case file is what tests/cast_common.py: dump_cases writes: four u32 { rays, spheres, planes, lights }, then the records (32, 96, 96 and 48
 * bytes each).  tests/test_paths_host.py writes the census rays of its scenes, with degenerate rays (zero, NaN and infinite directions, NaN
 * origins and tmax) behind them.  Every case runs with each combination of CLW_PATH_TRANSMIT x CLW_PATH_ALL_SURFACES x CLW_CAST_OPAQUE on
 * all three kinds, with 1, 2 and 8 segments, with and without `next`, on all rays at once and on the first rays one at a time.  The outputs
 * are allocated at exactly bounces * n hits, n bytes and n rays (a write beyond them is the address sanitizer's to report), and every answer
 * is held to the definition's own rules: count <= bounces, a known reason that fits the count, misses behind the count ... see check().  Prints one line per
 * run and "paths_sanitize: N runs, 0 failures"; exit status 1 on a failed check (a sanitizer report aborts).  Host code only: nothing here
 * touches a GPU.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "paths_host.h"

static int failures = 0, runs = 0;

static int is_miss(const clw_hit* h) {
    return h->t == INFINITY && h->id == CLW_ID_NONE && h->normal[0] == 0 && h->normal[1] == 0 && h->normal[2] == 0 && h->point[0] == 0 &&
           h->point[1] == 0 && h->point[2] == 0;
}

/* the rules an answer keeps whatever the scene is */
static int check(const clw_ray* rays, uint32_t n, uint32_t B, const clw_hit* hits, const uint8_t* status, const clw_ray* next, const clw_hit* first,
                 uint32_t reasons[3]) {
    int ok = 1;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t count = CLW_PATH_COUNT(status[i]), reason = CLW_PATH_REASON(status[i]);
        ok = ok && count <= B && reason <= 2u;
        if (reason == CLW_PATH_REASON_BOUNCES) ok = ok && count == B;
        if (reason == CLW_PATH_REASON_MISSED) ok = ok && count < B;
        if (reason == CLW_PATH_REASON_ENDED) ok = ok && count >= 1u;
        if (reason <= 2u) reasons[reason]++;
        for (uint32_t k = 0; k < B; k++) {
            const clw_hit* h = hits + (size_t)k * n + i;
            if (k < count) ok = ok && h->id != CLW_ID_NONE && !isnan(h->t) && h->t > 0 && h->t <= rays[i].tmax;
            else ok = ok && is_miss(h);
        }
        ok = ok && memcmp(hits + i, first + i, sizeof(clw_hit)) == 0;      /* segment 0 is the nearest-hit query */
        if (next) {
            if (reason == CLW_PATH_REASON_ENDED) ok = ok && next[i].dir[0] == 0 && next[i].dir[1] == 0 && next[i].dir[2] == 0 && next[i].ignore == CLW_ID_NONE;
            if (reason == CLW_PATH_REASON_MISSED && count == 0u) ok = ok && memcmp(next + i, rays + i, sizeof(clw_ray)) == 0;
            if (reason != CLW_PATH_REASON_MISSED || count > 0u) ok = ok && next[i].ignore == CLW_ID_NONE;
            ok = ok && memcmp(&next[i].tmax, &rays[i].tmax, 4) == 0;
        }
    }
    return ok;
}

static void run(const char* name, const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t B, int with_next, const uint8_t* sp, uint32_t ns,
                const uint8_t* pl, uint32_t np, const uint8_t* li, uint32_t nl, int quiet) {
    clw_hit* hits = (clw_hit*)malloc(sizeof(clw_hit) * (size_t)B * n);
    clw_hit* first = (clw_hit*)malloc(sizeof(clw_hit) * (size_t)n);
    uint8_t* status = (uint8_t*)malloc(n);
    clw_ray* next = with_next ? (clw_ray*)malloc(sizeof(clw_ray) * (size_t)n) : NULL;
    uint32_t reasons[3] = {0, 0, 0};
    int ok = hits && first && status && (next || !with_next) &&
             clw_host_cast_paths(rays, n, flags, B, sp, ns, pl, np, li, nl, hits, status, next) == 1 &&
             clw_host_cast_rays(rays, n, flags & WT_PATHS_CAST_FLAGS, sp, ns, pl, np, li, nl, first) == 1;
    ok = ok && check(rays, n, B, hits, status, next, first, reasons);
    runs++;
    if (!quiet || !ok)
        printf("%-24s n %4u flags %2u B %u next %d: %u reach B, %u miss, %u end%s\n", name, n, flags, B, with_next, reasons[0], reasons[1], reasons[2],
               ok ? "" : "  FAILED");
    if (!ok) failures++;
    free(hits); free(first); free(status); free(next);
}

static int run_file(const char* path) {
    FILE* f = fopen(path, "rb");
    uint32_t head[4];
    if (!f || fread(head, 4, 4, f) != 4) { printf("%s: cannot read  FAILED\n", path); if (f) fclose(f); return 0; }
    const uint32_t n = head[0], ns = head[1], np = head[2], nl = head[3];
    if (n == 0u || n > (1u << 20) || ns > (1u << 20) || np > (1u << 20) || nl > (1u << 20)) { printf("%s: bad header  FAILED\n", path); fclose(f); return 0; }
    clw_ray* rays = (clw_ray*)malloc(sizeof(clw_ray) * (size_t)n);
    uint8_t* sp = (uint8_t*)malloc(96 * (size_t)(ns ? ns : 1));
    uint8_t* pl = (uint8_t*)malloc(96 * (size_t)(np ? np : 1));
    uint8_t* li = (uint8_t*)malloc(48 * (size_t)(nl ? nl : 1));
    int ok = rays && sp && pl && li && fread(rays, sizeof(clw_ray), n, f) == n && fread(sp, 96, ns, f) == ns && fread(pl, 96, np, f) == np &&
             fread(li, 48, nl, f) == nl;
    fclose(f);
    if (!ok) printf("%s: short file  FAILED\n", path);
    const uint32_t Bs[3] = {1u, 2u, 8u};
    for (uint32_t combo = 0; ok && combo < 8u; combo++) {
        const uint32_t flags = CLW_CAST_KINDS | ((combo & 1u) ? CLW_PATH_TRANSMIT : 0u) | ((combo & 2u) ? CLW_PATH_ALL_SURFACES : 0u) |
                               ((combo & 4u) ? CLW_CAST_OPAQUE : 0u);
        for (int b = 0; b < 3; b++) {
            run(path, rays, n, flags, Bs[b], 1, sp, ns, pl, np, li, nl, 0);
            run(path, rays, n, flags, Bs[b], 0, sp, ns, pl, np, li, nl, 1);
            for (uint32_t i = 0; i < n && i < 24u; i++) run("one ray alone", rays + i, 1, flags, Bs[b], (int)(i & 1u), sp, ns, pl, np, li, nl, 1);
        }
    }
    /* refusals write nothing: the outputs are one byte long */
    uint8_t small[1] = {0xA5};
    if (ok) {
        runs++;
        if (clw_host_cast_paths(rays, n, CLW_CAST_KINDS, 0, sp, ns, pl, np, li, nl, (clw_hit*)small, small, NULL) != 0 ||
            clw_host_cast_paths(rays, n, CLW_CAST_KINDS, 9, sp, ns, pl, np, li, nl, (clw_hit*)small, small, NULL) != 0 ||
            clw_host_cast_paths(rays, n, 64u | 7u, 1, sp, ns, pl, np, li, nl, (clw_hit*)small, small, NULL) != 0 ||
            clw_host_cast_paths(rays, 0, CLW_CAST_KINDS, 1, sp, ns, pl, np, li, nl, (clw_hit*)small, small, NULL) != 0 || small[0] != 0xA5) {
            failures++;
            printf("%s: a refusal was accepted or wrote  FAILED\n", path);
        }
    }
    free(rays); free(sp); free(pl); free(li);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: paths_sanitize CASE.bin ...\n"); return 2; }
    for (int a = 1; a < argc; a++)
        if (!run_file(argv[a])) failures++;
    printf("paths_sanitize: %d runs, %d failures\n", runs, failures);
    return failures ? 1 : 0;
}
