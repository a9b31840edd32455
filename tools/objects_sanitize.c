/*
 * objects_sanitize.c -- the visible-object table's host model (csrc/objects_host.c) on the shapes of its unit test, as a stand-alone host
 * program for a sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -I example_gui_opencl_raytracer_amd/csrc \
 *       tools/objects_sanitize.c example_gui_opencl_raytracer_amd/csrc/objects_host.c -o objects_sanitize
 *   ./objects_sanitize
 *
 * Ids, depth and the output table are heap blocks of exactly the sizes the call is entitled to (so that a read or a write beyond them is the
 * address sanitizer's to report).  Every size runs first rows 0, 8 and 13, rectangles inside, across and beyond the range (64-bit clipping: x +
 * width beyond 2^32), fields with foreign ids, with and without depth, and capacities 0, 1 and exact; the result is held to: records ascending
 * by id, pixels adding up to summary.pixels - summary.foreign, every box inside the clipped rectangle, and a table split at a row merging into
 * the whole.  The refusals are called with a one-record table and a summary they must not touch.  Prints "objects_sanitize: N cases, 0
 * failures"; exit status 1 on a failed check (a sanitizer report aborts).  Host code only: nothing here touches a GPU.
 */
#include "objects_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t rng_state = 2463534242u;
static uint32_t next(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int failures = 0, cases = 0;
static const uint32_t COUNTS[3] = {8u, 2u, 3u};

static uint32_t some_id(void) {
    switch (next() % 6u) {
        case 0: return next() % 9u;                              /* a sphere; index 8 is foreign */
        case 1: return (1u << 30) | (next() % 3u);               /* a plane; index 2 is foreign */
        case 2: return (2u << 30) | (next() % 4u);               /* a light; index 3 is foreign */
        case 3: return CLW_ID_NONE;
        case 4: return (3u << 30) | (next() % 5u);               /* kind 3 that is not CLW_ID_NONE */
        default: return 5u;
    }
}

/* the table of a range into a block of exactly `objects` records -> the block (caller frees), the count through n */
static clw_object_stat* table_of(const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect,
                                 uint32_t* n, clw_object_summary* s) {
    clw_object_summary probe;
    if (!clw_host_object_stats(ids, depth, width, rows, first_row, rect, COUNTS, NULL, 0, &probe)) { *n = 0; failures++; return NULL; }
    clw_object_stat* out = (clw_object_stat*)malloc((probe.objects ? probe.objects : 1u) * sizeof *out);
    if (!clw_host_object_stats(ids, depth, width, rows, first_row, rect, COUNTS, out, probe.objects, s) || s->objects != probe.objects) failures++;
    *n = probe.objects;
    return out;
}

static void run(uint32_t width, uint32_t rows, uint32_t first_row) {
    const size_t n = (size_t)width * rows;
    uint32_t* ids = (uint32_t*)malloc(n * 4);
    float* depth = (float*)malloc(n * 4);
    for (size_t p = 0; p < n; p++) { ids[p] = some_id(); depth[p] = (float)(next() % 1000u) * 0.25f + 0.5f; }
    const clw_rect rects[] = {
        {0u, first_row, width, rows}, {width - 1u, first_row + rows - 1u, 1u, 1u}, {width / 3u, first_row + rows / 3u, width, rows + 5u},
        {width > 1u ? 1u : 0u, first_row > 3u ? first_row - 3u : 0u, 0xFFFFFFFFu, 0xFFFFFFFFu}, {0u, first_row + rows, width, 4u}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}};
    for (size_t k = 0; k <= sizeof rects / sizeof rects[0]; k++) {
        const clw_rect* rect = k ? &rects[k - 1] : NULL;
        for (int with_depth = 0; with_depth < 2; with_depth++) {
            const float* d = with_depth ? depth : NULL;
            uint32_t cnt, clip[4];
            clw_object_summary s;
            clw_object_stat* t = table_of(ids, d, width, rows, first_row, rect, &cnt, &s);
            int ok = t != NULL;
            const int hit = wt_objects_clip(width, rows, first_row, rect, clip);
            uint64_t pixels = 0;
            for (uint32_t i = 0; ok && i < cnt; i++) {
                pixels += t[i].pixels;
                ok = ok && (i == 0 || t[i - 1].id < t[i].id) && t[i].pixels > 0u;
                ok = ok && t[i].x0 >= clip[0] && t[i].x1 < clip[0] + clip[2] && t[i].x0 <= t[i].x1;
                ok = ok && t[i].y0 >= first_row + clip[1] && t[i].y1 < first_row + clip[1] + clip[3] && t[i].y0 <= t[i].y1;
                ok = ok && t[i].sum_x >= (uint64_t)t[i].x0 * t[i].pixels && t[i].sum_x <= (uint64_t)t[i].x1 * t[i].pixels;
                if (!with_depth) ok = ok && t[i].depth_min == 0.0f && t[i].depth_max == 0.0f;
            }
            ok = ok && pixels + s.foreign == s.pixels && s.pixels == (hit ? clip[2] * clip[3] : 0u) && (hit || cnt == 0u);
            /* a one-record capacity writes one record and reports them all */
            if (ok && cnt > 1u) {
                clw_object_stat* one = (clw_object_stat*)malloc(sizeof *one);
                clw_object_summary s1;
                ok = clw_host_object_stats(ids, d, width, rows, first_row, rect, COUNTS, one, 1, &s1) == 1 && s1.objects == cnt && !memcmp(one, t, sizeof *one);
                free(one);
            }
            /* split at the middle row, merged: the whole */
            if (ok && rows > 1u) {
                const uint32_t r = rows / 2u;
                uint32_t na, nb;
                clw_object_summary sa, sb;
                clw_object_stat* a = table_of(ids, d, width, r, first_row, rect, &na, &sa);
                clw_object_stat* b = table_of(ids + (size_t)r * width, d ? d + (size_t)r * width : NULL, width, rows - r, first_row + r, rect, &nb, &sb);
                clw_object_stat* m = (clw_object_stat*)malloc((cnt ? cnt : 1u) * sizeof *m);
                ok = clw_host_merge_object_stats(a, na, b, nb, m, cnt) == cnt && (cnt == 0u || !memcmp(m, t, cnt * sizeof *m));
                ok = ok && clw_host_merge_object_stats(b, nb, a, na, m, cnt) == cnt && (cnt == 0u || !memcmp(m, t, cnt * sizeof *m));
                free(a); free(b); free(m);
            }
            cases++;
            if (!ok) { failures++; printf("%u x %u first row %u rectangle %u depth %d  FAILED\n", width, rows, first_row, (unsigned)k, with_depth); }
            free(t);
        }
    }
    free(ids); free(depth);
}

static void refuse(const char* what, const uint32_t* ids, uint32_t width, uint32_t rows, const clw_rect* rect, const uint32_t* counts, int with_summary) {
    clw_object_stat* out = (clw_object_stat*)malloc(sizeof *out);
    clw_object_summary s = {7u, 7u, 7u, 7u};
    memset(out, 0xA5, sizeof *out);
    const int ok = clw_host_object_stats(ids, NULL, width, rows, 0, rect, counts, out, 1, with_summary ? &s : NULL) == 0 && out->id == 0xA5A5A5A5u &&
                   s.objects == 7u && s.pixels == 7u;
    cases++;
    if (!ok) { failures++; printf("refusal: %s  FAILED\n", what); }
    free(out);
}

int main(void) {
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {31, 7}, {33, 9}, {61, 43}, {130, 17}, {1, 300}, {300, 1}};
    const uint32_t first_rows[] = {0u, 8u, 13u};
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++)
        for (size_t f = 0; f < 3; f++) run(sizes[i][0], sizes[i][1], first_rows[f]);

    uint32_t* one = (uint32_t*)calloc(1, 4);
    const clw_rect flat = {0u, 0u, 0u, 1u}, thin = {0u, 0u, 1u, 0u};
    const uint32_t many[3] = {(1u << 24) - 2u, 1u, 1u}, wrap[3] = {0xFFFFFFFFu, 1u, 0u};
    refuse("no ids", NULL, 1, 1, NULL, COUNTS, 1);
    refuse("no counts", one, 1, 1, NULL, NULL, 1);
    refuse("no summary", one, 1, 1, NULL, COUNTS, 0);
    refuse("zero width", one, 0, 1, NULL, COUNTS, 1);
    refuse("zero rows", one, 1, 0, NULL, COUNTS, 1);
    refuse("a rectangle of zero width", one, 1, 1, &flat, COUNTS, 1);
    refuse("a rectangle of zero height", one, 1, 1, &thin, COUNTS, 1);
    refuse("2^24 + 1 slots", one, 1, 1, NULL, many, 1);
    refuse("counts beyond 32 bits", one, 1, 1, NULL, wrap, 1);
    refuse("2^30 pixels", one, 1u << 15, 1u << 15, NULL, COUNTS, 1);
    free(one);
    printf("objects_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
