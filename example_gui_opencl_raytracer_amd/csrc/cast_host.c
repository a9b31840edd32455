/* cast_host.c -- THE definition of the ray queries (include/hip_wrap_ext.h: clw_host_cast_rays, clw_host_occluded_rays): the device pass
 * (wt_cast: whitted_cast.inc) is held to it bit for bit.  Written for reading, not for speed: every ray on its own against every primitive that
 * takes part, the rules in the header's order.  wt_cast_enumerate is the one copy of that rule: the queries here and the layered ones
 * (layers_host.c) differ only in what they do with a candidate.  The arithmetic -- the two hit tests, the winner's point and normal -- is
 * ref_tests.h, the one text the device pass is compiled from too.  Built with -ffp-contract=off: every float32 operation is rounded once. */
#include "cast_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ref_tests.h"
#include "scene_prep.h"

int wt_cast_check(uint32_t n, uint32_t flags) {
    if (n == 0u || n >= (1u << 30)) return 0;
    if (flags & ~(CLW_CAST_KINDS | CLW_CAST_OPAQUE)) return 0;
    if (!(flags & CLW_CAST_KINDS)) return 0;
    return 1;
}

int wt_cast_enumerate(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                      const void* lights, uint32_t nl, const wt_cast_visitor* v) {
    if (!wt_cast_check(n, flags) || !rays || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights)) return 0;
    /* the words the device reads: {centre, +-r * r} per sphere, {n, .}, {p0, .} per plane, {centre, r * r}, {.} per light (whitted_params.h) */
    const size_t f4 = wprep_geom_f4(ns, np, nl);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32 * (size_t)(np ? np : 1));
    if (!geom || !ptex) { free(geom); free(ptex); return 0; }
    wprep_build((const uint8_t*)spheres, ns, (const uint8_t*)planes, np, (const uint8_t*)lights, nl, geom, ptex);
    const wt_cast_geom g = {geom, geom + 4 * (size_t)ns, geom + 4 * (size_t)ns + 8 * (size_t)np};
    for (uint32_t k = 0; k < n; k++) {
        const ref_v3 o = ref_ld(rays[k].origin), d = ref_ld(rays[k].dir);
        const float tmax = rays[k].tmax;
        const uint32_t ignore = rays[k].ignore;
        float t;
        v->ray_begin(v->ctx);
        if (flags & CLW_CAST_SPHERES)
            for (uint32_t i = 0; i < ns; i++) {
                const float* s = g.spheres + 4 * (size_t)i;
                if (i == ignore || ((flags & CLW_CAST_OPAQUE) && sign_bit(s[3]))) continue;
                if (ref_sphere(o, d, ref_ld(s), s[3], &t) && t <= tmax) v->take(v->ctx, t, i);
            }
        if (flags & CLW_CAST_PLANES)
            for (uint32_t i = 0; i < np; i++) {
                if (((1u << 30) | i) == ignore) continue;
                if (ref_plane(o, d, ref_ld(g.planes + 8 * (size_t)i), ref_ld(g.planes + 8 * (size_t)i + 4), &t) && t <= tmax) v->take(v->ctx, t, (1u << 30) | i);
            }
        if (flags & CLW_CAST_LIGHTS)
            for (uint32_t i = 0; i < nl; i++) {
                if (((2u << 30) | i) == ignore) continue;
                const float* l = g.lights + 8 * (size_t)i;
                if (ref_sphere(o, d, ref_ld(l), l[3], &t) && t <= tmax) v->take(v->ctx, t, (2u << 30) | i);
            }
        v->ray_done(v->ctx, k, rays + k, &g);
    }
    free(geom);
    free(ptex);
    return 1;
}

/* both queries: the nearest candidate so far and whether there is one; hits != NULL the nearest is written, blocked != NULL the flag */
typedef struct { clw_hit* hits; uint8_t* blocked; float tbest; uint32_t best; int any; } nearest;

static void nearest_begin(void* ctx) {
    nearest* s = (nearest*)ctx;
    s->tbest = INFINITY; s->best = CLW_ID_NONE; s->any = 0;
}

static void nearest_take(void* ctx, float t, uint32_t id) {
    nearest* s = (nearest*)ctx;
    s->any = 1;
    if (t < s->tbest) { s->tbest = t; s->best = id; }
}

static void nearest_done(void* ctx, uint32_t k, const clw_ray* ray, const wt_cast_geom* g) {
    nearest* s = (nearest*)ctx;
    const float tbest = s->tbest;
    const uint32_t best = s->best;
    if (s->blocked) s->blocked[k] = (uint8_t)s->any;
    if (!s->hits) return;
    clw_hit* h = s->hits + k;
    h->t = tbest;
    h->id = best;
    for (int a = 0; a < 3; a++) { h->normal[a] = 0.0f; h->point[a] = 0.0f; }
    if (best == CLW_ID_NONE) return;
    const uint32_t kind = best >> 30, index = best & 0x3FFFFFFFu;
    /* the plane's normal, or the centre of the sphere or light */
    const float* w = kind == 1u ? g->planes + 8 * (size_t)index : kind == 0u ? g->spheres + 4 * (size_t)index : g->lights + 8 * (size_t)index;
    const ref_v3 point = ref_hit_point(ref_ld(ray->origin), ref_ld(ray->dir), tbest);
    ref_st(h->point, point);
    ref_st(h->normal, ref_hit_normal(kind == 1u, point, ref_ld(w)));
}

static int cast(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                const void* lights, uint32_t nl, clw_hit* hits, uint8_t* blocked) {
    nearest s = {hits, blocked, INFINITY, CLW_ID_NONE, 0};
    const wt_cast_visitor v = {nearest_begin, nearest_take, nearest_done, &s};
    return wt_cast_enumerate(rays, n, flags, spheres, ns, planes, np, lights, nl, &v);
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
