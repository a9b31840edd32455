/*
 * grid_sanitize.c -- the uniform-grid builder (csrc/scene_prep.c) on degenerate scenes, as a stand-alone host program for a sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fsanitize=float-cast-overflow -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/grid_sanitize.c example_gui_opencl_raytracer_amd/csrc/scene_prep.c -lm -o grid_sanitize
 *   ./grid_sanitize
 *
 * Every scene is planned with reg_pad 0 and 0.25; a scene the builder accepts is filled into tables of exactly the sizes the builder asked
 * for (so that a write beyond them is the address sanitizer's to report) and its tables are held to start[ncells] == pairs, items < ns.
 * Prints one line per case and "grid_sanitize: N cases, 0 failures"; exit status 1 on a failed check (a sanitizer report aborts).
 * Host code only: nothing here touches a GPU.
 */
#include "scene_prep.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_PAIRS ((size_t)1 << 25)

static uint32_t rng_state = 12345u;
static float uniform(float lo, float hi) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return lo + (hi - lo) * (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

static uint8_t* cloud(uint32_t ns, float box, float rlo, float rhi) {
    uint8_t* s = (uint8_t*)calloc(ns, 96);
    for (uint32_t i = 0; i < ns; i++) {
        float v[4] = {uniform(-box, box), uniform(-box, box), uniform(-box, box), 0.0f};
        float r = uniform(rlo, rhi);
        memcpy(s + 96 * (size_t)i, v, 16);
        memcpy(s + 96 * (size_t)i + 16, &r, 4);
    }
    return s;
}
static void set_f(uint8_t* s, uint32_t i, size_t off, float v) { memcpy(s + 96 * (size_t)i + off, &v, 4); }

static int failures = 0, cases = 0;

static void run(const char* name, const uint8_t* s, uint32_t ns, int expect_refused) {
    const float pads[2] = {0.0f, 0.25f};
    for (int k = 0; k < 2; k++) {
        wprep_grid g;
        memset(&g, 0xAB, sizeof g);
        size_t pairs = wprep_grid_plan(s, ns, 1.6f, pads[k], &g);
        int refused = pairs > MAX_PAIRS, ok = refused == expect_refused;
        cases++;
        if (!refused) {
            uint32_t* start = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)g.ncells + 1));
            uint32_t* items = (uint32_t*)malloc(sizeof(uint32_t) * (pairs ? pairs : 1));
            uint32_t* box = (uint32_t*)malloc(sizeof(uint32_t) * 2 * (size_t)ns);
            wprep_grid_fill(s, ns, &g, start, items, box);
            ok = ok && start[0] == 0 && start[g.ncells] == pairs;
            for (size_t e = 0; e < pairs; e++) ok = ok && items[e] < ns;
            for (int a = 0; a < 3; a++) ok = ok && g.res[a] >= 1 && g.res[a] <= 1024 && isfinite(g.cell[a]) && g.cell[a] > 0.0f;
            free(start); free(items); free(box);
            printf("%-28s pad %.2f: res %d x %d x %d, %zu pairs%s\n", name, pads[k], g.res[0], g.res[1], g.res[2], pairs, ok ? "" : "  FAILED");
        } else {
            printf("%-28s pad %.2f: no grid (linear scan)%s\n", name, pads[k], ok ? "" : "  FAILED");
        }
        if (!ok) failures++;
    }
}

int main(void) {
    uint8_t* s;
    s = cloud(300, 5.0f, 0.05f, 0.5f); run("cloud", s, 300, 0); free(s);
    s = cloud(257, 5.0f, 0.0f, 0.0f); run("radius 0", s, 257, 0); free(s);
    s = cloud(300, 0.0f, 0.7f, 0.7f); run("one sphere 300 times", s, 300, 0); free(s);
    s = cloud(300, 0.0f, 0.0f, 0.0f); run("one point 300 times", s, 300, 0); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 17, 4, NAN); run("NaN centre", s, 300, 1); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 200, 8, -INFINITY); run("infinite centre", s, 300, 1); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 5, 16, INFINITY); run("infinite radius", s, 300, 1); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 299, 16, NAN); run("NaN radius", s, 300, 1); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 100, 16, 1e30f); run("radius 1e30", s, 300, 0); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 100, 16, -0.4f); run("negative radius", s, 300, 0); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); set_f(s, 5, 16, 3e38f); set_f(s, 5, 0, 3e38f); run("bounds beyond a float", s, 300, 1); free(s);
    s = cloud(300, 5.0f, 0.05f, 0.5f); for (uint32_t i = 0; i < 300; i += 2) set_f(s, i, 0, 1e30f); run("two groups 1e30 apart", s, 300, 0); free(s);
    s = cloud(600, 0.0f, 0.3f, 0.3f); for (uint32_t i = 0; i < 600; i++) set_f(s, i, 0, 2.5f * (float)i); run("line 1500 long (1024 clamp)", s, 600, 0); free(s);
    s = cloud(300, 5.0f, 1e-30f, 1e-30f); run("radius 1e-30", s, 300, 0); free(s);
    s = cloud(300, 1e-20f, 1e-22f, 1e-21f); run("scene 1e-20 across", s, 300, 0); free(s);
    run("no spheres", NULL, 0, 1);
    printf("grid_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
