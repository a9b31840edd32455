/* cast_host.c -- THE definition of the ray queries (include/hip_wrap_ext.h: clw_host_cast_rays, clw_host_occluded_rays): the device pass
 * (wt_cast: whitted_cast.inc) is held to it bit for bit.  Written for reading, not for speed: every ray on its own against every primitive that
 * takes part, the rules in the header's order.  Built with -ffp-contract=off: every float32 operation below is rounded once. */
#include "cast_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "scene_prep.h"

int wt_cast_check(uint32_t n, uint32_t flags) {
    if (n == 0u || n >= (1u << 30)) return 0;
    if (flags & ~(CLW_CAST_KINDS | CLW_CAST_OPAQUE)) return 0;
    if (!(flags & CLW_CAST_KINDS)) return 0;
    return 1;
}

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* the primary-hit pass's evaluation of its winner (whitted_gbuffer.inc: wt_gb_ref_sphere, wt_gb_ref_plane), the same operations in C */
static int ref_sphere(const float o[3], const float d[3], const float s[4], float* t) {
    const float a = dot3(d, d);
    const float v[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
    const float c = dot3(v, v) - fabsf(s[3]);
    const float b = dot3(v, d);
    const float D = b * b + (-(a * c));
    const float sD = sqrtf(D);
    const float t0 = (-b - sD) / a;
    *t = (t0 < 0) ? (-b + sD) / a : t0;
    return !(D < 0) && !(*t <= 0);
}
static int ref_plane(const float o[3], const float d[3], const float n[4], const float p0[4], float* t) {
    const float w[3] = {p0[0] - o[0], p0[1] - o[1], p0[2] - o[2]};
    const float num = dot3(w, n);
    const float b = dot3(d, n);
    *t = num / b;
    return !(b == 0) && !(*t <= 0);
}

static int sign_bit(float f) { uint32_t u; memcpy(&u, &f, 4); return (int)(u >> 31); }

/* both queries: hits != NULL the nearest, blocked != NULL whether a candidate exists */
static int cast(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                const void* lights, uint32_t nl, clw_hit* hits, uint8_t* blocked) {
    if (!wt_cast_check(n, flags) || !rays || (!hits && !blocked) || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights)) return 0;
    /* the words the device reads: {centre, +-r * r} per sphere, {n, .}, {p0, .} per plane, {centre, r * r}, {.} per light (whitted_params.h) */
    const size_t f4 = wprep_geom_f4(ns, np, nl);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32 * (size_t)(np ? np : 1));
    if (!geom || !ptex) { free(geom); free(ptex); return 0; }
    wprep_build((const uint8_t*)spheres, ns, (const uint8_t*)planes, np, (const uint8_t*)lights, nl, geom, ptex);
    const float* pl = geom + 4 * (size_t)ns;
    const float* lg = pl + 8 * (size_t)np;
    for (uint32_t k = 0; k < n; k++) {
        const float* o = rays[k].origin;
        const float* d = rays[k].dir;
        const float tmax = rays[k].tmax;
        const uint32_t ignore = rays[k].ignore;
        float tbest = INFINITY, t;
        uint32_t best = CLW_ID_NONE;
        int any = 0;
        if (flags & CLW_CAST_SPHERES)
            for (uint32_t i = 0; i < ns; i++) {
                const float* s = geom + 4 * (size_t)i;
                if (i == ignore || ((flags & CLW_CAST_OPAQUE) && sign_bit(s[3]))) continue;
                if (ref_sphere(o, d, s, &t) && t <= tmax) { any = 1; if (t < tbest) { tbest = t; best = i; } }
            }
        if (flags & CLW_CAST_PLANES)
            for (uint32_t i = 0; i < np; i++) {
                if (((1u << 30) | i) == ignore) continue;
                if (ref_plane(o, d, pl + 8 * (size_t)i, pl + 8 * (size_t)i + 4, &t) && t <= tmax) { any = 1; if (t < tbest) { tbest = t; best = (1u << 30) | i; } }
            }
        if (flags & CLW_CAST_LIGHTS)
            for (uint32_t i = 0; i < nl; i++) {
                if (((2u << 30) | i) == ignore) continue;
                if (ref_sphere(o, d, lg + 8 * (size_t)i, &t) && t <= tmax) { any = 1; if (t < tbest) { tbest = t; best = (2u << 30) | i; } }
            }
        if (blocked) blocked[k] = (uint8_t)any;
        if (!hits) continue;
        clw_hit* h = hits + k;
        h->t = tbest;
        h->id = best;
        for (int a = 0; a < 3; a++) { h->normal[a] = 0.0f; h->point[a] = 0.0f; }
        if (best == CLW_ID_NONE) continue;
        for (int a = 0; a < 3; a++) h->point[a] = d[a] * tbest + o[a];
        const uint32_t kind = best >> 30, index = best & 0x3FFFFFFFu;
        if (kind == 1u) {
            for (int a = 0; a < 3; a++) h->normal[a] = pl[8 * (size_t)index + a];
        } else {
            const float* c = kind == 0u ? geom + 4 * (size_t)index : lg + 8 * (size_t)index;
            const float w[3] = {h->point[0] - c[0], h->point[1] - c[1], h->point[2] - c[2]};
            const float len = sqrtf(dot3(w, w));
            for (int a = 0; a < 3; a++) h->normal[a] = w[a] / len;
        }
    }
    free(geom);
    free(ptex);
    return 1;
}

int clw_host_cast_rays(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                       const void* lights, uint32_t nl, clw_hit* hits) {
    if (!hits) return 0;
    return cast(rays, n, flags, spheres, ns, planes, np, lights, nl, hits, NULL);
}

int clw_host_occluded_rays(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                           const void* lights, uint32_t nl, uint8_t* blocked) {
    if (!blocked) return 0;
    return cast(rays, n, flags, spheres, ns, planes, np, lights, nl, NULL, blocked);
}
