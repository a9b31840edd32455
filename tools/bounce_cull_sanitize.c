/*
 * bounce_cull_sanitize.c -- the bounce cull table's definition (csrc/bounce_cull_host.c: clw_host_bounce_cull) on degenerate inputs, as a
 * stand-alone host program for a sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -ffp-contract=off -D_DEFAULT_SOURCE -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/bounce_cull_sanitize.c example_gui_opencl_raytracer_amd/csrc/bounce_cull_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/primary_cull_host.c example_gui_opencl_raytracer_amd/csrc/host_camera.c \
 *       example_gui_opencl_raytracer_amd/csrc/scene_prep.c -lm -o bounce_cull_sanitize
 *   ./bounce_cull_sanitize
 *
 * A floor, a wall, four spheres and three lights seen from a small camera; then each term in turn made zero, NaN, infinite or huge: camera
 * terms, plane normals and points, sphere and light centres and radii; no spheres, no planes, nine planes (more than the rule looks at), no
 * lights; frames of one pixel, of one row, widths that are no multiple of 8; row strips and band shares; depth 0 and 1; every `parts`.  The
 * output is allocated at exactly the tile count (a write beyond it is the address sanitizer's to report).  Held: the return value is the tile
 * count (or 0 for a refused call, which writes nothing), no byte has bits 6-7, no byte is set where the primary byte lacks bit 0, a camera
 * term that is not finite writes zeros, depth < 2 sets no reflected bit.  Prints one line per case and "bounce_cull_sanitize: N cases, 0
 * failures"; exit status 1 on a failed check (a sanitizer report aborts).  Host code only: nothing here touches a GPU.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/hip_wrap_ext.h"
#include "bounce_cull_host.h"

enum { NS = 4, NP = 9, NL = 3 };
static int failures = 0, cases = 0;
static uint8_t sp[NS * 96], pl[NP * 96], li[NL * 48];

static void put(uint8_t* rec, size_t off, float v) { memcpy(rec + off, &v, 4); }
static void put3(uint8_t* rec, size_t off, float x, float y, float z) { put(rec, off, x); put(rec, off + 4, y); put(rec, off + 8, z); }

static void base_scene(void) {
    memset(sp, 0, sizeof sp); memset(pl, 0, sizeof pl); memset(li, 0, sizeof li);
    put3(sp, 0, 4.5f, 0.5f, -1.0f); put(sp, 16, 0.5f);
    put3(sp + 96, 0, -1.0f, 1.0f, 4.5f); put(sp + 96, 16, 0.8f);
    put3(sp + 192, 0, 0.8f, 0.8f, 1.5f); put(sp + 192, 16, 0.8f);
    put3(sp + 288, 0, -0.6f, 0.8f, -1.0f); put(sp + 288, 16, 0.8f);
    put3(pl, 0, 0, 1, 0);                                       /* the floor y = 0 */
    put3(pl + 96, 0, 0, 0, -1); put3(pl + 96, 16, 0, 0, 7);     /* the wall z = 7 */
    for (int i = 2; i < NP; i++) { put3(pl + 96 * i, 0, 0, -1, 0); put3(pl + 96 * i, 16, 0, 20.0f + (float)i, 0); }      /* ceilings */
    put3(li, 0, -2, 3, 2); put(li, 16, 0.1f); put(li, 20, 8.0f);
    put3(li + 48, 0, 2, 1.5f, 0.2f); put(li + 48, 16, 0.1f); put(li + 48, 20, 50.0f);
    put3(li + 96, 0, 1, 4, 3); put(li + 96, 16, 0.1f); put(li + 96, 20, 20.0f);
}

static void run(const char* name, const clw_camera* cam, uint32_t row_offset, uint32_t rows, uint32_t stride, uint32_t phase, uint32_t ns, uint32_t np,
                uint32_t nl, uint32_t depth, uint32_t parts, int expect_refused, int expect_zero) {
    const uint32_t tiles = wt_cull_tiles(cam->width, rows);
    uint8_t* out = (uint8_t*)malloc(tiles ? tiles : 1);
    uint8_t* prim = (uint8_t*)malloc(tiles ? tiles : 1);
    memset(out, 0xC0, tiles ? tiles : 1);
    const uint32_t n = clw_host_bounce_cull(cam, row_offset, rows, stride, phase, ns ? sp : NULL, ns, np ? pl : NULL, np, nl ? li : NULL, nl, depth, parts, out);
    int ok = expect_refused ? n == 0u : n == tiles;
    unsigned set = 0;
    if (ok && n) {
        ok = clw_host_primary_cull(cam, row_offset, rows, stride, phase, ns ? sp : NULL, ns, nl ? li : NULL, nl, prim) == n;
        for (uint32_t t = 0; ok && t < n; t++) {
            ok = !(out[t] & 0xC0u) && (!out[t] || (prim[t] & 1u)) && !(depth < 2u && (out[t] & 48u)) && !(!(parts & 1u) && (out[t] & 15u)) &&
                 !(!(parts & 2u) && (out[t] & 48u)) && !(expect_zero && out[t]);
            set += out[t] != 0;
        }
    }
    if (ok && !n) for (uint32_t t = 0; t < tiles; t++) ok = ok && out[t] == 0xC0u;      /* refused: nothing written */
    cases++;
    printf("%-44s %3u tiles, %3u with bits%s\n", name, n, set, ok ? "" : "  FAILED");
    if (!ok) failures++;
    free(out); free(prim);
}

int main(void) {
    const float origin[3] = {0.8f, 2.5f, -8.0f}, look[3] = {0.2f, 0.0f, 1.0f};
    const float bad[6] = {0.0f, NAN, INFINITY, -INFINITY, 3e38f, 1e-38f};
    clw_camera cam;
    char name[96];
    base_scene();
    if (!clw_host_perspective(origin, look, 90.0f, 1.0f, 77, 45, &cam)) { printf("clw_host_perspective refused the camera  FAILED\n"); return 1; }
    run("the scene", &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 0);
    for (uint32_t parts = 0; parts < 4; parts++) { snprintf(name, sizeof name, "parts %u", parts); run(name, &cam, 0, 45, 1, 0, NS, 2, NL, 4, parts, 0, 0); }
    for (uint32_t depth = 0; depth < 3; depth++) { snprintf(name, sizeof name, "depth %u", depth); run(name, &cam, 0, 45, 1, 0, NS, 2, NL, depth, 3, 0, 0); }
    run("no spheres", &cam, 0, 45, 1, 0, 0, 2, NL, 4, 3, 0, 0);
    run("no planes", &cam, 0, 45, 1, 0, NS, 0, NL, 4, 3, 0, 1);
    run("no lights", &cam, 0, 45, 1, 0, NS, 2, 0, 4, 3, 0, 0);
    run("eight planes", &cam, 0, 45, 1, 0, NS, 8, NL, 4, 3, 0, 0);
    run("nine planes: more than the rule reads", &cam, 0, 45, 1, 0, NS, 9, NL, 4, 3, 0, 1);
    run("a row strip", &cam, 13, 21, 1, 0, NS, 2, NL, 4, 3, 0, 0);
    run("a band share", &cam, 0, 16, 3, 2, NS, 2, NL, 4, 3, 0, 0);
    run("band phase beyond the stride", &cam, 0, 16, 3, 3, NS, 2, NL, 4, 3, 1, 0);
    run("no rows", &cam, 0, 0, 1, 0, NS, 2, NL, 4, 3, 1, 0);
    run("one row", &cam, 44, 1, 1, 0, NS, 2, NL, 4, 3, 0, 0);
    { clw_camera c = cam; c.width = 1; run("a frame one pixel wide", &c, 0, 1, 1, 0, NS, 2, NL, 4, 3, 0, 0); }
    { clw_camera c = cam; c.width = 0; run("no columns", &c, 0, 8, 1, 0, NS, 2, NL, 4, 3, 1, 0); }
    for (int b = 0; b < 6; b++) {
        for (int f = 0; f < 6; f++) {
            clw_camera c = cam;
            float* terms[6] = {&c.im_corner[1], &c.origin[2], &c.up[0], &c.right[1], &c.w_factor, &c.h_factor};
            *terms[f] = bad[b];
            snprintf(name, sizeof name, "camera term %d = %g", f, (double)bad[b]);
            run(name, &c, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, !isfinite(bad[b]));
        }
        for (int p = 0; p < 2; p++) for (int w = 0; w < 2; w++) for (int a = 0; a < 3; a++) {
            base_scene();
            put(pl + 96 * p, (w ? 16 : 0) + 4 * (size_t)a, bad[b]);
            snprintf(name, sizeof name, "plane %d %s[%d] = %g", p, w ? "point" : "normal", a, (double)bad[b]);
            run(name, &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 0);
        }
        for (int w = 0; w < 4; w++) {
            base_scene();
            put(sp + 96 * 2, w < 3 ? 4 * (size_t)w : 16, bad[b]);
            snprintf(name, sizeof name, "sphere 2 word %d = %g", w, (double)bad[b]);
            run(name, &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 0);
            base_scene();
            put(li + 48, w < 3 ? 4 * (size_t)w : 16, bad[b]);
            snprintf(name, sizeof name, "light 1 word %d = %g", w, (double)bad[b]);
            run(name, &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 0);
        }
    }
    base_scene();
    put3(pl, 0, 0, 0, 0);
    run("a zero normal", &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 1);
    base_scene();
    memcpy(pl + 96, pl, 96);
    run("the same plane twice", &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 1);
    base_scene();
    put3(li, 0, 0.8f, 2.5f, -8.0f);
    run("a light on the camera", &cam, 0, 45, 1, 0, NS, 2, NL, 4, 3, 0, 0);
    if (clw_host_bounce_cull(NULL, 0, 45, 1, 0, sp, NS, pl, 2, li, NL, 4, 3, sp) != 0 || clw_host_bounce_cull(&cam, 0, 45, 1, 0, NULL, NS, pl, 2, li, NL, 4, 3, sp) != 0 ||
        clw_host_bounce_cull(&cam, 0, 45, 1, 0, sp, NS, NULL, 2, li, NL, 4, 3, sp) != 0 || clw_host_bounce_cull(&cam, 0, 45, 1, 0, sp, NS, pl, 2, li, NL, 4, 3, NULL) != 0) {
        failures++;
        printf("a missing pointer was not refused  FAILED\n");
    }
    cases++;
    printf("bounce_cull_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
