/* bounce_cull_host.c -- THE definition of the bounce cull table (include/hip_wrap_ext.h: clw_host_bounce_cull; the rule and its margins:
 * bounce_cull_host.h).  The device builder (wt_primary_cull_build: whitted_cull.inc) compiles the same wt_bc_tile and is held to this table
 * bit for bit.  Built with -ffp-contract=off: every operation is rounded once. */
#include "bounce_cull_host.h"

#include <stdlib.h>
#include <string.h>

#include "../../include/hip_wrap_ext.h"
#include "scene_prep.h"

uint32_t wt_bc_table(const wt_cull_view* V, const wt_bc_scene* S, uint32_t parts, uint8_t* prim, uint8_t* out) {
    const uint32_t n = V ? wt_cull_tiles(V->width, V->rows) : 0u;
    if (n == 0u || !out || !S || (S->ns > 0u && !S->spheres) || (S->nl > 0u && !S->lights) || (S->np > 0u && (!S->planes || !S->planes_raw))) return 0u;
    memset(out, 0, n);
    if (prim) memset(prim, 0, n);
    if (!wt_cull_view_ok(V)) return n;
    const uint32_t tpr = (V->width + 7u) / 8u;
    for (uint32_t t = 0; t < n; t++) {
        const uint8_t p = wt_cull_tile(V, t % tpr, t / tpr, S->spheres, S->ns, S->lights, S->nl);
        if (prim) prim[t] = p;
        out[t] = wt_bc_tile(V, t % tpr, t / tpr, p, S, parts);
    }
    return n;
}

uint32_t clw_host_bounce_cull(const clw_camera* cam, uint32_t row_offset, uint32_t rows, uint32_t band_stride, uint32_t band_phase, const void* spheres,
                              uint32_t ns, const void* planes, uint32_t np, const void* lights, uint32_t nl, uint32_t depth, uint32_t parts, uint8_t* out) {
    if (!cam || !out || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights) || wt_cull_tiles(cam->width, rows) == 0u) return 0u;
    if (band_stride > 1u && band_phase >= band_stride) return 0u;
    wt_cull_view V;
    memcpy(V.corner, cam->im_corner, sizeof V.corner); memcpy(V.origin, cam->origin, sizeof V.origin);
    memcpy(V.up, cam->up, sizeof V.up); memcpy(V.right, cam->right, sizeof V.right);
    V.w_factor = cam->w_factor; V.h_factor = cam->h_factor;
    V.width = cam->width; V.rows = rows; V.row_offset = row_offset; V.band_stride = band_stride; V.band_phase = band_phase;
    const size_t f4 = wprep_geom_f4(ns, np, nl);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32 * ((size_t)np ? (size_t)np : 1));
    uint32_t* raw = (uint32_t*)malloc(96 * ((size_t)np ? (size_t)np : 1));      /* an aligned copy of the records: the rule reads a word of each */
    if (!geom || !ptex || !raw) { free(geom); free(ptex); free(raw); return 0u; }
    if (np) memcpy(raw, planes, 96 * (size_t)np);
    wprep_build((const uint8_t*)spheres, ns, (const uint8_t*)planes, np, (const uint8_t*)lights, nl, geom, ptex);
    const wt_bc_scene S = {geom, geom + 4 * (size_t)ns, geom + 4 * ((size_t)ns + 2 * (size_t)np), raw, ns, np, nl, depth};
    const uint32_t n = wt_bc_table(&V, &S, parts, NULL, out);
    free(geom); free(ptex); free(raw);
    return n;
}
