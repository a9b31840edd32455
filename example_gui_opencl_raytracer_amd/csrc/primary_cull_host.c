/* primary_cull_host.c -- THE definition of the primary-ray cull table (include/hip_wrap_ext.h: clw_host_primary_cull; the rule and its margin:
 * primary_cull_host.h).  The device builder (wt_primary_cull_build: whitted_cull.inc) compiles the same wt_cull_tile and is held to this table
 * bit for bit.  Built with -ffp-contract=off: every operation below is rounded once. */
#include "primary_cull_host.h"

#include <stdlib.h>
#include <string.h>

#include "../../include/hip_wrap_ext.h"
#include "scene_prep.h"

uint32_t wt_cull_tiles(uint32_t width, uint32_t rows) {
    const uint64_t n = (((uint64_t)width + 7u) / 8u) * (((uint64_t)rows + 7u) / 8u);
    return (width == 0u || rows == 0u || n >= (1ull << 31)) ? 0u : (uint32_t)n;
}

uint32_t wt_cull_table(const wt_cull_view* V, const float* spheres, uint32_t ns, const float* lights, uint32_t nl, uint8_t* out) {
    const uint32_t n = V ? wt_cull_tiles(V->width, V->rows) : 0u;
    if (n == 0u || !out || (ns > 0u && !spheres) || (nl > 0u && !lights)) return 0u;
    memset(out, 0, n);
    if (!wt_cull_view_ok(V)) return n;
    const uint32_t tpr = (V->width + 7u) / 8u;
    for (uint32_t t = 0; t < n; t++) out[t] = wt_cull_tile(V, t % tpr, t / tpr, spheres, ns, lights, nl);
    return n;
}

uint32_t clw_host_primary_cull(const clw_camera* cam, uint32_t row_offset, uint32_t rows, uint32_t band_stride, uint32_t band_phase, const void* spheres,
                               uint32_t ns, const void* lights, uint32_t nl, uint8_t* out) {
    if (!cam || !out || (ns > 0u && !spheres) || (nl > 0u && !lights) || wt_cull_tiles(cam->width, rows) == 0u) return 0u;
    if (band_stride > 1u && band_phase >= band_stride) return 0u;
    wt_cull_view V;
    memcpy(V.corner, cam->im_corner, sizeof V.corner); memcpy(V.origin, cam->origin, sizeof V.origin);
    memcpy(V.up, cam->up, sizeof V.up); memcpy(V.right, cam->right, sizeof V.right);
    V.w_factor = cam->w_factor; V.h_factor = cam->h_factor;
    V.width = cam->width; V.rows = rows; V.row_offset = row_offset; V.band_stride = band_stride; V.band_phase = band_phase;
    /* the words the device reads: {centre, +-r * r} per sphere, {centre, r * r}, {.} per light (whitted_params.h) */
    const size_t f4 = wprep_geom_f4(ns, 0u, nl);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32);
    if (!geom || !ptex) { free(geom); free(ptex); return 0u; }
    wprep_build((const uint8_t*)spheres, ns, NULL, 0u, (const uint8_t*)lights, nl, geom, ptex);
    const uint32_t n = wt_cull_table(&V, geom, ns, geom + 4 * (size_t)ns, nl, out);
    free(geom);
    free(ptex);
    return n;
}
