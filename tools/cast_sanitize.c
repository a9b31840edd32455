/*
 * cast_sanitize.c -- the ray queries' host definition (csrc/cast_host.c, with csrc/scene_prep.c) on the ray sets of the host test, as a
 * stand-alone host program for a sanitizer build:
 *
 *   PYTHONPATH=.:tests python -c "import cast_common as cc; cc.dump_cases('/tmp/cast_cases')"
 *   gcc -O1 -g -std=c99 -D_DEFAULT_SOURCE -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/cast_sanitize.c example_gui_opencl_raytracer_amd/csrc/cast_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/scene_prep.c -lm -o cast_sanitize
 *   ./cast_sanitize /tmp/cast_cases/*.bin
 *
 * A case file is what tests/cast_common.py's dump_cases writes for a scene of the host test: four u32 { rays, spheres, planes, lights }, then
 * the clw_ray records, the 96-byte sphere and plane records and the 48-byte light records.  Rays, scene arrays, hits and blocked bytes are
 * heap blocks of exactly the sizes the call is entitled to (so that a read or a write beyond them is the address sanitizer's to report).
 * Every case runs all 14 flag words that name a kind, nearest and any, with the file's rays and again with the first ray alone (n = 1); the
 * result is held to: blocked == (id != CLW_ID_NONE), a miss is {+inf, CLW_ID_NONE, 0, 0}, a hit's index lies inside its array.  The refusals
 * are called with output blocks of ONE byte, which they must not touch.  Prints "cast_sanitize: N cases, 0 failures"; exit status 1 on a
 * failed check (a sanitizer report aborts).
 * Host code only: nothing here touches a GPU.
 */
#include "cast_host.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures = 0, cases = 0;

static void* block(FILE* f, size_t bytes) {      /* exactly `bytes` bytes of the file; NULL for none */
    if (!bytes) return NULL;
    void* p = malloc(bytes);
    if (!p || fread(p, 1, bytes, f) != bytes) { printf("short case file\n"); exit(1); }
    return p;
}

static void run(const char* path, const clw_ray* rays, uint32_t n, const void* sp, uint32_t ns, const void* pl, uint32_t np, const void* li,
                uint32_t nl) {
    for (uint32_t flags = 1; flags < 16; flags++) {
        if (!(flags & CLW_CAST_KINDS)) continue;
        clw_hit* hits = (clw_hit*)malloc((size_t)n * sizeof(clw_hit));
        uint8_t* blocked = (uint8_t*)malloc(n);
        int ok = clw_host_cast_rays(rays, n, flags, sp, ns, pl, np, li, nl, hits) == 1 &&
                 clw_host_occluded_rays(rays, n, flags, sp, ns, pl, np, li, nl, blocked) == 1;
        for (uint32_t k = 0; ok && k < n; k++) {
            const clw_hit* h = hits + k;
            const uint32_t kind = h->id >> 30, index = h->id & 0x3FFFFFFFu;
            ok = ok && blocked[k] == (h->id != CLW_ID_NONE);
            if (h->id == CLW_ID_NONE) ok = ok && isinf(h->t) && h->t > 0 && !h->normal[0] && !h->normal[1] && !h->normal[2] && !h->point[0] && !h->point[1] && !h->point[2];
            else ok = ok && h->t > 0 && h->t <= rays[k].tmax && h->id != rays[k].ignore && (flags & (1u << kind)) && index < (kind == 0 ? ns : kind == 1 ? np : nl);
        }
        cases++;
        if (!ok) { failures++; printf("%s n %u flags %u  FAILED\n", path, n, flags); }
        free(hits); free(blocked);
    }
}

static void refuse(const char* what, const clw_ray* rays, uint32_t n, uint32_t flags, const void* sp, uint32_t ns, const void* pl, uint32_t np,
                   const void* li, uint32_t nl, int with_out) {
    uint8_t* out = (uint8_t*)malloc(1);
    out[0] = 0xA5;
    const int ok = clw_host_cast_rays(rays, n, flags, sp, ns, pl, np, li, nl, with_out ? (clw_hit*)out : NULL) == 0 &&
                   clw_host_occluded_rays(rays, n, flags, sp, ns, pl, np, li, nl, with_out ? out : NULL) == 0 && out[0] == 0xA5;
    cases++;
    if (!ok) { failures++; printf("refusal: %s  FAILED\n", what); }
    free(out);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: cast_sanitize CASE.bin ...\n"); return 1; }
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        uint32_t head[4];
        if (!f || fread(head, 4, 4, f) != 4) { printf("cannot read %s\n", argv[a]); return 1; }
        const uint32_t n = head[0], ns = head[1], np = head[2], nl = head[3];
        clw_ray* rays = (clw_ray*)block(f, (size_t)n * sizeof(clw_ray));
        void* sp = block(f, 96 * (size_t)ns);
        void* pl = block(f, 96 * (size_t)np);
        void* li = block(f, 48 * (size_t)nl);
        fclose(f);
        run(argv[a], rays, n, sp, ns, pl, np, li, nl);
        clw_ray* one = (clw_ray*)malloc(sizeof(clw_ray));      /* n = 1: a block of one ray */
        memcpy(one, rays, sizeof(clw_ray));
        run(argv[a], one, 1, sp, ns, pl, np, li, nl);
        if (a == 1) {
            refuse("no rays", NULL, 1, 3, sp, ns, pl, np, li, nl, 1);
            refuse("no output", one, 1, 3, sp, ns, pl, np, li, nl, 0);
            refuse("n = 0", one, 0, 3, sp, ns, pl, np, li, nl, 1);
            refuse("n = 1 << 30", one, 1u << 30, 3, sp, ns, pl, np, li, nl, 1);
            refuse("no kind", one, 1, CLW_CAST_OPAQUE, sp, ns, pl, np, li, nl, 1);
            refuse("unknown flag bit", one, 1, 16u | 3u, sp, ns, pl, np, li, nl, 1);
            if (ns) refuse("spheres without their array", one, 1, 3, NULL, ns, pl, np, li, nl, 1);
            if (np) refuse("planes without their array", one, 1, 3, sp, ns, NULL, np, li, nl, 1);
            if (nl) refuse("lights without their array", one, 1, 3, sp, ns, pl, np, NULL, nl, 1);
        }
        free(one); free(rays); free(sp); free(pl); free(li);
    }
    printf("cast_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
