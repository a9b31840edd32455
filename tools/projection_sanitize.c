/*
 * projection_sanitize.c -- the host definition of the camera models beside the pinhole (csrc/projection_host.c) on the sizes of the tests,
 * as a stand-alone host program for a sanitizer build:
 *
 *   gcc -O1 -g -std=c99 -D_DEFAULT_SOURCE -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       -I example_gui_opencl_raytracer_amd/csrc tools/projection_sanitize.c example_gui_opencl_raytracer_amd/csrc/projection_host.c \
 *       example_gui_opencl_raytracer_amd/csrc/host_camera.c -o projection_sanitize -lm
 *   ./projection_sanitize
 *
 * The record buffer and the two tables are heap blocks of exactly the sizes a call is entitled to (so that a read or a write beyond them is
 * the address sanitizer's to report): whole frames and sub-ranges of 67 x 45, 64 x 32, 9 x 1 and 1 x 1, all three models.  The results are
 * held to: zero padding words, unit directions, one direction for the orthographic view, the camera origin for the panorama.  The refusals
 * are called with a block of ONE record, which they must not touch.  Prints "projection_sanitize: N cases, 0 failures"; exit status 1 on a
 * failed check (a sanitizer report aborts).  Host code only: nothing here touches a GPU.
 */
#include "projection_host.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures = 0, cases = 0;

static void check(int ok, const char* what, uint32_t w, uint32_t h) {
    cases++;
    if (!ok) { failures++; printf("FAILED: %s at %u x %u\n", what, (unsigned)w, (unsigned)h); }
}

static void run(uint32_t w, uint32_t h) {
    const float origin[3] = {0.8f, 2.5f, -8.0f}, look[3] = {0.2f, -0.15f, 1.0f};
    clw_camera pin, ortho;
    clw_projection po, pe, pp;
    check(clw_host_perspective(origin, look, 90.0f, 1.0f, w, h, &pin) == 1, "perspective", w, h);
    check(clw_host_ortho_camera(origin, look, 12.0f, w, h, &ortho, &po) == 1, "ortho_camera", w, h);
    memset(&pe, 0, sizeof pe); memset(&pp, 0, sizeof pp);
    pe.model = CLW_PROJ_EQUIRECT; pe.h_span = 200.0f; pe.v_span = 90.0f;
    pp.model = CLW_PROJ_PERSPECTIVE;
    const uint64_t total = (uint64_t)w * h;
    const uint64_t ranges[3][2] = {{0, total}, {total / 3, total - total / 4}, {total - 1, total}};
    const struct { const clw_camera* cam; const clw_projection* proj; } views[3] = {{&ortho, &po}, {&pin, &pe}, {&pin, &pp}};
    for (int v = 0; v < 3; v++)
        for (int r = 0; r < 3; r++) {
            const uint64_t a = ranges[r][0], b = ranges[r][1], n = b - a;
            float* rays = (float*)malloc(n ? (size_t)n * 64 : 1);      /* exactly n records */
            int ok = clw_host_projection_rays(views[v].cam, views[v].proj, a, b, rays) == 1;
            for (uint64_t i = 0; ok && i < n; i++) {
                const float* q = rays + 16 * i;
                const double len = sqrt((double)q[4] * q[4] + (double)q[5] * q[5] + (double)q[6] * q[6]);
                ok = ok && fabs(len - 1.0) <= 1.0 / (1 << 22) && q[3] == 0.0f && q[7] == 0.0f;
                for (int k = 8; k < 16; k++) ok = ok && q[k] == 0.0f;
                if (v == 0) ok = ok && !memcmp(q + 4, rays + 4, 12);
                else ok = ok && !memcmp(q, origin, 12);
            }
            check(ok, v == 0 ? "ortho rays" : v == 1 ? "equirect rays" : "pinhole rays", w, h);
            free(rays);
        }
    float* col = (float*)malloc((size_t)w * 16);      /* exactly w and h float4 */
    float* row = (float*)malloc((size_t)h * 16);
    check(clw_host_projection_tables(&pin, &pe, col, row) == 1, "tables", w, h);
    check(clw_host_projection_tables(&ortho, &po, col, row) == 0, "tables of another model", w, h);
    free(col); free(row);
}

static void refusals(void) {
    const float origin[3] = {0, 0, 0}, look[3] = {0, 0, 1}, up_y[3] = {0, 1, 0};
    clw_camera pin, flat;
    clw_projection p, q;
    float* one = (float*)malloc(64);
    memset(one, 0x5A, 64);
    clw_host_perspective(origin, look, 90.0f, 1.0f, 4, 4, &pin);
    clw_host_ortho_camera(origin, look, 2.0f, 4, 4, &flat, &q);
    memset(&p, 0, sizeof p);
    int refused = 1;
    p.model = 3; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.model = CLW_PROJ_ORTHO; p.reserved = 1; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.reserved = 0; p.ortho_width = -1.0f; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.ortho_width = NAN; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.ortho_width = 0.0f; p.h_span = 361.0f; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.h_span = 0.0f; p.v_span = INFINITY; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.v_span = 0.0f; p.axis[1] = NAN; refused &= !clw_host_projection_rays(&pin, &p, 0, 1, one);
    p.axis[1] = 0.0f; refused &= !clw_host_projection_rays(&flat, &p, 0, 1, one);      /* zero axis, zero centre direction */
    refused &= !clw_host_projection_rays(&pin, &p, 2, 1, one) && !clw_host_projection_rays(&pin, &p, 0, 17, one);
    refused &= !clw_host_projection_rays(NULL, &p, 0, 1, one) && !clw_host_projection_rays(&pin, NULL, 0, 1, one) && !clw_host_projection_rays(&pin, &p, 0, 1, NULL);
    refused &= !clw_host_ortho_camera(origin, up_y, 2.0f, 4, 4, &flat, &q) && !clw_host_ortho_camera(origin, look, 0.0f, 4, 4, &flat, &q) &&
               !clw_host_ortho_camera(origin, look, 2.0f, 0, 4, &flat, &q);
    for (int k = 0; k < 64; k++) refused &= ((unsigned char*)one)[k] == 0x5A;
    check(refused, "refusals leave the block alone", 4, 4);
    free(one);
}

int main(void) {
    const uint32_t sizes[4][2] = {{67, 45}, {64, 32}, {9, 1}, {1, 1}};
    for (int s = 0; s < 4; s++) run(sizes[s][0], sizes[s][1]);
    refusals();
    printf("projection_sanitize: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
