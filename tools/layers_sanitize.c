/*
 * layers_sanitize.c -- the layered ray queries' definition (csrc/layers_host.c: clw_host_cast_layers, clw_host_camera_rays) on degenerate rays,
 * as a stand-alone host program for a sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -ffp-contract=off -D_DEFAULT_SOURCE -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/layers_sanitize.c example_gui_opencl_raytracer_amd/csrc/layers_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/cast_host.c example_gui_opencl_raytracer_amd/csrc/projection_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/host_camera.c example_gui_opencl_raytracer_amd/csrc/scene_prep.c -lm -o layers_sanitize
 *   ./layers_sanitize
 *
 * A scene of 14 spheres on a line (two coincident), a plane and a light; rays with zero, NaN and infinite directions, NaN origins, NaN, zero,
 * negative and infinite tmax beside ordinary ones along the line; K = 1 and K = 8, n = 1 and n = all.  The outputs are allocated at exactly
 * K * n words (a write beyond them is the address sanitizer's to report), and every answer is held to the definition's own rules: keys ascend
 * strictly, empty entries follow the listed ones and are {+inf, CLW_ID_NONE}, no t is NaN, the lists for K = 1 are a prefix of those for K = 8,
 * and layer 0 is clw_host_cast_rays' {t, id} where that t is finite.  The camera rays of the three models over a few id ranges are held to
 * tmax = +inf, ignore = CLW_ID_NONE.  Prints one line per case and "layers_sanitize: N cases, 0 failures"; exit status 1 on a failed check (a
 * sanitizer report aborts).  Host code only: nothing here touches a GPU.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "layers_host.h"

enum { NS = 14, NP = 1, NL = 1 };
static int failures = 0, cases = 0;

static void put(uint8_t* rec, size_t off, float v) { memcpy(rec + off, &v, 4); }

static clw_ray ray(float ox, float oy, float oz, float dx, float dy, float dz, float tmax, uint32_t ignore) {
    clw_ray r = {{ox, oy, oz}, tmax, {dx, dy, dz}, ignore};
    return r;
}

static int check_lists(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, const float* t, const uint32_t* id, const float* t8, const uint32_t* id8,
                       const clw_hit* hits) {
    int ok = 1;
    (void)rays; (void)flags;
    for (uint32_t i = 0; i < n; i++) {
        for (uint32_t k = 0; k < K; k++) {
            const float tk = t[(size_t)k * n + i];
            const uint32_t ik = id[(size_t)k * n + i];
            ok = ok && !isnan(tk) && (ik == CLW_ID_NONE) == (tk == INFINITY);
            if (k > 0) {
                const float tp = t[(size_t)(k - 1) * n + i];
                const uint32_t ip = id[(size_t)(k - 1) * n + i];
                ok = ok && (ik == CLW_ID_NONE ? 1 : (ip != CLW_ID_NONE && (tp < tk || (tp == tk && ip < ik))));
            }
            if (t8) ok = ok && memcmp(&tk, &t8[(size_t)k * n + i], 4) == 0 && ik == id8[(size_t)k * n + i];
        }
        if (hits && isfinite(hits[i].t)) ok = ok && memcmp(&hits[i].t, &t[i], 4) == 0 && hits[i].id == id[i];
        if (hits && !isfinite(hits[i].t)) ok = ok && id[i] == CLW_ID_NONE;
    }
    return ok;
}

static void run(const char* name, const clw_ray* rays, uint32_t n, uint32_t flags, const uint8_t* sp, const uint8_t* pl, const uint8_t* li) {
    float* t8 = (float*)malloc(4 * (size_t)8 * n);
    uint32_t* id8 = (uint32_t*)malloc(4 * (size_t)8 * n);
    float* t1 = (float*)malloc(4 * (size_t)n);
    uint32_t* id1 = (uint32_t*)malloc(4 * (size_t)n);
    clw_hit* hits = (clw_hit*)malloc(sizeof(clw_hit) * (size_t)n);
    int ok = clw_host_cast_layers(rays, n, flags, 8, sp, NS, pl, NP, li, NL, t8, id8) == 1 &&
             clw_host_cast_layers(rays, n, flags, 1, sp, NS, pl, NP, li, NL, t1, id1) == 1 &&
             clw_host_cast_rays(rays, n, flags, sp, NS, pl, NP, li, NL, hits) == 1;
    ok = ok && check_lists(rays, n, flags, 8, t8, id8, NULL, NULL, hits) && check_lists(rays, n, flags, 1, t1, id1, t8, id8, hits);
    uint32_t listed = 0, full = 0;
    for (uint32_t i = 0; ok && i < n; i++) { listed += id8[i] != CLW_ID_NONE; full += id8[(size_t)7 * n + i] != CLW_ID_NONE; }
    cases++;
    printf("%-34s n %3u flags %2u: %u rays list something, %u fill 8 layers%s\n", name, n, flags, listed, full, ok ? "" : "  FAILED");
    if (!ok) failures++;
    free(t8); free(id8); free(t1); free(id1); free(hits);
}

int main(void) {
    uint8_t* sp = (uint8_t*)calloc(NS, 96);
    uint8_t* pl = (uint8_t*)calloc(NP, 96);
    uint8_t* li = (uint8_t*)calloc(NL, 48);
    for (uint32_t i = 0; i < NS; i++) {      /* {origin (16 bytes), radius} as the scene arrays start; the material stays zero */
        put(sp + 96 * (size_t)i, 0, 2.0f * (float)(i == 9 ? 4 : i));      /* sphere 9 on sphere 4 */
        put(sp + 96 * (size_t)i, 4, 1.0f);
        put(sp + 96 * (size_t)i, 16, i == 6 ? -0.6f : 0.6f);
    }
    put(pl, 0, 1.0f); put(pl, 16, -3.0f);      /* normal (1, 0, 0) through (-3, 0, 0) */
    put(li, 0, 40.0f); put(li, 4, 1.0f); put(li, 16, 0.5f);

    const float nan = NAN, inf = INFINITY;
    clw_ray rays[24];
    uint32_t n = 0;
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, inf, CLW_ID_NONE);            /* along the line: 17 candidates */
    rays[n++] = ray(50, 1, 0, -2, 0, 0, inf, 4);                     /* back, the twin of the ignored sphere stays */
    rays[n++] = ray(8, 1, 0, 1, 0, 0, 7.5f, CLW_ID_NONE);            /* from inside the coincident pair, ending on the way */
    rays[n++] = ray(-6, 1, 0, 0, 0, 0, inf, CLW_ID_NONE);            /* zero direction */
    rays[n++] = ray(-6, 1, 0, nan, 0, 0, inf, CLW_ID_NONE);          /* NaN direction */
    rays[n++] = ray(-6, 1, 0, 1, nan, nan, inf, CLW_ID_NONE);
    rays[n++] = ray(-6, 1, 0, inf, 0, 0, inf, CLW_ID_NONE);          /* infinite direction */
    rays[n++] = ray(-6, 1, 0, -inf, inf, 0, 1.0f, CLW_ID_NONE);
    rays[n++] = ray(nan, 1, 0, 1, 0, 0, inf, CLW_ID_NONE);           /* NaN origin */
    rays[n++] = ray(inf, 1, 0, -1, 0, 0, inf, CLW_ID_NONE);          /* infinite origin */
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, nan, CLW_ID_NONE);            /* NaN tmax */
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, 0.0f, CLW_ID_NONE);           /* tmax 0, negative, -inf */
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, -1.0f, CLW_ID_NONE);
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, -inf, CLW_ID_NONE);
    rays[n++] = ray(-6, 1, 0, 1e-30f, 0, 0, inf, CLW_ID_NONE);       /* t overflows to +inf: candidates that are not listed */
    rays[n++] = ray(-6, 1, 0, 1e30f, 0, 0, inf, CLW_ID_NONE);        /* d.d overflows */
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, inf, (1u << 30) | 0u);        /* the plane ignored */
    rays[n++] = ray(-6, 1, 0, 1, 0, 0, inf, 0x7FFFFFFFu);            /* an id no primitive has */
    rays[n++] = ray(3e38f, 3e38f, 0, -1, -1, 0, inf, CLW_ID_NONE);   /* products beyond a float */

    const uint32_t flag_sets[5] = {1u, 2u, 4u, 7u, 15u};
    for (int f = 0; f < 5; f++) {
        run("every ray", rays, n, flag_sets[f], sp, pl, li);
        for (uint32_t i = 0; i < n; i++) {
            char name[48];
            snprintf(name, sizeof name, "ray %u alone", i);
            run(name, rays + i, 1, flag_sets[f], sp, pl, li);
        }
    }

    /* the camera rays: the three models, the whole frame, a strip, one pixel, an empty range; a refused projection writes nothing */
    clw_camera cam;
    const float origin[3] = {0, 4, -6}, look[3] = {0, -0.2f, 1};
    int have = clw_host_perspective(origin, look, 80.0f, 1.0f, 13, 7, &cam);
    for (uint32_t model = 0; have && model < 3; model++) {
        clw_projection proj;
        memset(&proj, 0, sizeof proj);
        proj.model = model;
        proj.axis[2] = model ? 1.0f : 0.0f;
        const uint64_t ranges[4][2] = {{0, 91}, {13, 39}, {45, 46}, {7, 7}};
        for (int r = 0; r < 4; r++) {
            const uint64_t b = ranges[r][0], e = ranges[r][1];
            clw_ray* out = (clw_ray*)malloc(sizeof(clw_ray) * (size_t)(e - b ? e - b : 1));
            int ok = clw_host_camera_rays(&cam, &proj, b, e, out) == 1;
            for (uint64_t i = 0; ok && i < e - b; i++) ok = out[i].tmax == INFINITY && out[i].ignore == CLW_ID_NONE && isfinite(out[i].dir[0]) && isfinite(out[i].origin[1]);
            cases++;
            printf("camera rays model %u ids [%llu, %llu)%s\n", model, (unsigned long long)b, (unsigned long long)e, ok ? "" : "  FAILED");
            if (!ok) failures++;
            free(out);
        }
        clw_ray none;
        cases++;
        if (clw_host_camera_rays(&cam, &proj, 0, 92, &none) != 0 || clw_host_camera_rays(&cam, &proj, 5, 4, &none) != 0) { failures++; printf("camera rays model %u: a range outside the frame was not refused  FAILED\n", model); }
    }
    if (!have) { failures++; printf("clw_host_perspective refused the camera  FAILED\n"); }
    free(sp); free(pl); free(li);
    printf("layers_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
