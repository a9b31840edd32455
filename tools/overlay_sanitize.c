/*
 * overlay_sanitize.c -- the selection overlay's host model (csrc/overlay_host.c) on its edge sizes, as a stand-alone host program for a
 * sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -I example_gui_opencl_raytracer_amd/csrc \
 *       tools/overlay_sanitize.c example_gui_opencl_raytracer_amd/csrc/overlay_host.c -o overlay_sanitize
 *   ./overlay_sanitize
 *
 * Frame, ids, selection and output are heap blocks of exactly the sizes the call is entitled to (so that a read or a write beyond them is the
 * address sanitizer's to report): 1 x 1, one row, one column, widths and heights around the outline's radius, the sizes of the unit test.
 * Every size runs all 7 flag words at radius 1 and 4 with 0, 1 and 64 ids; the result is held to: top byte 0, a selected pixel never takes
 * the outline's colour by rule 4, alpha 256 paints fill_rgb.  The refusals are called with an output block of ONE word, which they must not
 * touch.  Prints "overlay_sanitize: N cases, 0 failures"; exit status 1 on a failed check (a sanitizer report aborts).
 * Host code only: nothing here touches a GPU.
 */
#include "overlay_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t rng_state = 2463534242u;
static uint32_t next(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int failures = 0, cases = 0;

static void run(uint32_t width, uint32_t rows) {
    const size_t n = (size_t)width * rows;
    uint32_t* frame = (uint32_t*)malloc(n * 4);
    uint32_t* ids = (uint32_t*)malloc(n * 4);
    uint32_t* out = (uint32_t*)malloc(n * 4);
    const uint32_t counts[3] = {0u, 1u, 64u};
    for (size_t p = 0; p < n; p++) { frame[p] = next(); ids[p] = next() % 3u ? next() % 70u : CLW_ID_NONE; }
    for (int c = 0; c < 3; c++) {
        const uint32_t count = counts[c];
        uint32_t* sel = count ? (uint32_t*)malloc(count * 4) : NULL;      /* exactly `count` words */
        for (uint32_t k = 0; k < count; k++) sel[k] = k == 0 ? CLW_ID_NONE : k;
        for (uint32_t flags = 1; flags <= CLW_OV_ALL; flags++) {
            for (uint32_t radius = 1; radius <= 4; radius += 3) {
                const clw_overlay st = {flags, radius, 0x00FFFF00u, 0xFF123456u, 256u, 0x0000FF40u};
                int ok = clw_host_overlay(frame, ids, width, rows, &st, sel, count, out) == 1;
                for (size_t p = 0; ok && p < n; p++) {
                    int selected = 0;
                    for (uint32_t k = 0; k < count; k++) selected |= ids[p] == sel[k];
                    ok = ok && (out[p] >> 24) == 0u;
                    if ((flags & CLW_OV_FILL) && selected) ok = ok && out[p] == 0x00123456u;
                    if (flags == CLW_OV_OUTLINE && selected) ok = ok && out[p] == (frame[p] & 0x00FFFFFFu);
                }
                cases++;
                if (!ok) { failures++; printf("%u x %u flags %u radius %u count %u  FAILED\n", width, rows, flags, radius, count); }
            }
        }
        free(sel);
    }
    free(frame); free(ids); free(out);
}

static void refuse(const char* what, const uint32_t* frame, const uint32_t* ids, uint32_t width, uint32_t rows, const clw_overlay* st,
                   const uint32_t* sel, uint32_t count) {
    uint32_t* out = (uint32_t*)malloc(4);
    out[0] = 0xA5A5A5A5u;
    const int ok = clw_host_overlay(frame, ids, width, rows, st, sel, count, out) == 0 && out[0] == 0xA5A5A5A5u;
    cases++;
    if (!ok) { failures++; printf("refusal: %s  FAILED\n", what); }
    free(out);
}

int main(void) {
    const uint32_t sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {4, 4}, {5, 3}, {3, 5}, {8, 8}, {9, 9}, {61, 43}, {64, 16}, {130, 17}, {1, 300}, {300, 1}};
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++) run(sizes[i][0], sizes[i][1]);

    uint32_t* one = (uint32_t*)calloc(1, 4);
    uint32_t* sel = (uint32_t*)calloc(64, 4);      /* 64 words: a refused count of 65 must not read the 65th */
    const clw_overlay good = {7u, 2u, 1u, 2u, 96u, 3u};
    clw_overlay st;
    st = good; st.flags = 8u; refuse("unknown flag bit", one, one, 1, 1, &st, sel, 1);
    st = good; st.flags = 0u; refuse("no flag", one, one, 1, 1, &st, sel, 1);
    st = good; st.radius = 0u; refuse("radius 0", one, one, 1, 1, &st, sel, 1);
    st = good; st.radius = 5u; refuse("radius 5", one, one, 1, 1, &st, sel, 1);
    st = good; st.fill_alpha = 257u; refuse("alpha 257", one, one, 1, 1, &st, sel, 1);
    refuse("65 ids", one, one, 1, 1, &good, sel, 65);
    refuse("ids without their array", one, one, 1, 1, &good, NULL, 1);
    refuse("zero width", one, one, 0, 1, &good, sel, 1);
    refuse("zero rows", one, one, 1, 0, &good, sel, 1);
    refuse("no style", one, one, 1, 1, NULL, sel, 1);
    free(one); free(sel);
    printf("overlay_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
