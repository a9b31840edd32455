/* ao_host.c -- THE definition of the ambient occlusion pass (include/hip_wrap_ext.h: clw_host_ao_dirs, clw_host_ao_open, clw_host_ao_resolve):
 * the device pass (wt_ao_trace, wt_ao_resolve: whitted_ao.inc) is held to it bit for bit.  Written for reading, not for speed: every pixel on
 * its own, every ray against every primitive, the rules in the header's order.  The arithmetic -- the two hit tests, the basis of a normal,
 * a ray's direction, the integers of the resolve -- is ref_tests.h, the one text the device pass is compiled from too.  Built with
 * -ffp-contract=off: every float32 operation is rounded once. */
#include "ao_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ref_tests.h"
#include "scene_prep.h"

int wt_ao_check(const clw_ao* ao) {
    if (!ao) return 0;
    if (ao->flags & ~(CLW_AO_FILTER | CLW_AO_COMPOSE)) return 0;
    if (ao->rays < 1u || ao->rays > WT_AO_MAX_RAYS) return 0;
    if (!(ao->radius > 0.0f)) return 0;      /* NaN, 0 and negative; +inf passes */
    if (ao->strength > 256u) return 0;
    return 1;
}

int wt_ao_range_ok(uint32_t width, uint32_t rows) {
    return width != 0u && rows != 0u && (uint64_t)width * rows < (1ull << 30);
}

/* ---- (a) the direction table -------------------------------------------------------------------------------------------------------- */
int clw_host_ao_dirs(uint32_t K, float* dirs4) {
    if (!dirs4 || K < 1u || K > WT_AO_MAX_RAYS) return 0;
    for (uint32_t j = 0; j < WT_AO_PATTERNS; j++) {
        const uint32_t rev4 = ((j & 1u) << 3) | ((j & 2u) << 1) | ((j & 4u) >> 1) | ((j & 8u) >> 3);
        for (uint32_t i = 0; i < K; i++) {
            const double u1 = ((double)i + ((double)j + 0.5) / 16.0) / (double)K;
            const double s = (double)i * 0.6180339887498949 + (double)rev4 / 16.0;
            const double u2 = s - floor(s);
            const double r = sqrt(u1), phi = 2.0 * 3.14159265358979323846 * u2;
            float* l = dirs4 + 4 * ((size_t)j * K + i);
            l[0] = (float)(r * cos(phi));
            l[1] = (float)(r * sin(phi));
            l[2] = (float)sqrt(1.0 - u1);
            l[3] = 0.0f;
        }
    }
    return 1;
}

/* ---- (b) the open rays of every pixel ----------------------------------------------------------------------------------------------- */
int clw_host_ao_open(const float* point, const float* normal, const uint32_t* ids, uint32_t width, uint32_t rows, uint32_t first_row,
                     const void* spheres, uint32_t ns, const void* planes, uint32_t np, const clw_ao* ao, const float* dirs4,
                     uint8_t* open_u8) {
    if (!wt_ao_check(ao) || !wt_ao_range_ok(width, rows) || !point || !normal || !ids || !dirs4 || !open_u8 || (ns > 0u && !spheres) ||
        (np > 0u && !planes))
        return 0;
    /* the words the device reads: {centre, +-r * r} per sphere, {n, .}, {p0, .} per plane (whitted_params.h) */
    const size_t f4 = wprep_geom_f4(ns, np, 0u);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32 * (size_t)(np ? np : 1));
    if (!geom || !ptex) { free(geom); free(ptex); return 0; }
    wprep_build((const uint8_t*)spheres, ns, (const uint8_t*)planes, np, NULL, 0u, geom, ptex);
    const float* pl = geom + 4 * (size_t)ns;
    const uint32_t K = ao->rays;
    const float radius = ao->radius;
    for (uint32_t y = 0; y < rows; y++) {
        for (uint32_t x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            const uint32_t id = ids[p], kind = id >> 30, index = id & 0x3FFFFFFFu;
            if (!((kind == 0u && index < ns) || (kind == 1u && index < np))) { open_u8[p] = (uint8_t)K; continue; }
            const ref_v3 o = ref_ld(point + 3 * p), n = ref_ld(normal + 3 * p);
            ref_v3 t, u;
            ref_ao_basis(n, &t, &u);
            const uint32_t j = (x & 3u) | (((first_row + y) & 3u) << 2);
            uint32_t open = 0u;
            for (uint32_t i = 0; i < K; i++) {
                const float* l = dirs4 + 4 * ((size_t)j * K + i);
                const ref_v3 d = ref_ao_dir(t, u, n, l[0], l[1], l[2]);
                int occluded = 0;
                float th;
                for (uint32_t s = 0; s < ns; s++)
                    if (ref_sphere(o, d, ref_ld(geom + 4 * (size_t)s), geom[4 * (size_t)s + 3], &th) && th <= radius) occluded = 1;
                for (uint32_t q = 0; q < np; q++)
                    if (ref_plane(o, d, ref_ld(pl + 8 * (size_t)q), ref_ld(pl + 8 * (size_t)q + 4), &th) && th <= radius) occluded = 1;
                if (!occluded) open++;
            }
            open_u8[p] = (uint8_t)open;
        }
    }
    free(geom);
    free(ptex);
    return 1;
}

/* ---- (c) counts -> pixels, integers only -------------------------------------------------------------------------------------------- */
int clw_host_ao_resolve(const uint8_t* open_u8, const uint32_t* ids, const uint32_t* frame, uint32_t width, uint32_t rows, const clw_ao* ao,
                        uint32_t* out_u32) {
    if (!wt_ao_check(ao) || !wt_ao_range_ok(width, rows) || !open_u8 || !ids || !out_u32 || ((ao->flags & CLW_AO_COMPOSE) && !frame)) return 0;
    const uint32_t K = ao->rays;
    for (uint32_t y = 0; y < rows; y++) {
        for (uint32_t x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            uint32_t S = open_u8[p], m = 1u;
            if (ao->flags & CLW_AO_FILTER) {
                S = 0u; m = 0u;
                const uint32_t x0 = x > 2u ? x - 2u : 0u, x1 = x + 1u < width ? x + 1u : width - 1u;
                const uint32_t y0 = y > 2u ? y - 2u : 0u, y1 = y + 1u < rows ? y + 1u : rows - 1u;
                for (uint32_t qy = y0; qy <= y1; qy++)
                    for (uint32_t qx = x0; qx <= x1; qx++) {
                        const size_t q = (size_t)qy * width + qx;
                        if (ids[q] == ids[p]) { S += open_u8[q]; m++; }
                    }
            }
            const uint32_t vs = ref_ao_level(S, m, K, ao->strength);
            out_u32[p] = (ao->flags & CLW_AO_COMPOSE) ? ref_ao_compose(frame[p], vs) : ref_ao_grey(vs);
        }
    }
    return 1;
}
