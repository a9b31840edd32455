/* near_host.c -- THE definition of the proximity queries (include/hip_wrap_ext.h: clw_host_nearest_surface, clw_host_within_reach,
 * clw_host_near_surfaces): the device pass (wt_near: whitted_near.inc) is held to it bit for bit.  Written for reading, not for speed: every
 * probe on its own against every primitive that takes part, the rules in the header's order.  The arithmetic -- the two distances, the
 * winner's point and normal -- is ref_tests.h, the one text the device pass is compiled from too; the list rule is layers_host.c's.  Built with
 * -ffp-contract=off: every float32 operation is rounded once. */
#include "near_host.h"

#include <math.h>
#include <stdlib.h>

#include "cast_host.h"
#include "layers_host.h"
#include "ref_tests.h"
#include "scene_prep.h"

int wt_near_check(uint32_t n, uint32_t flags) { return wt_cast_check(n, flags); }
int wt_near_list_check(uint32_t n, uint32_t flags, uint32_t K) { return wt_layers_check(n, flags, K); }

/* what a probe keeps of its candidates: the nearest and whether there is one (hits / within), or the K nearest (K > 0) */
typedef struct {
    clw_hit* hits; uint8_t* within; float* d_out; uint32_t* id_out; uint32_t K;
    float best; uint32_t best_id; int any;
    wt_layer_list L;
} near_sink;

static void take(near_sink* s, float d, uint32_t id) {
    s->any = 1;
    if (d < s->best) { s->best = d; s->best_id = id; }      /* (an equal d keeps the earlier primitive) */
    if (s->K) wt_layers_candidate(&s->L, d, id);
}

static int near_enumerate(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                          const void* planes, uint32_t np, const void* lights, uint32_t nl, near_sink* s) {
    if (!wt_near_check(n, flags) || !probes || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights)) return 0;
    /* the words the device reads: {centre, +-r * r} per sphere, {n, .}, {p0, .} per plane, {centre, r * r}, {.} per light (whitted_params.h) */
    const size_t f4 = wprep_geom_f4(ns, np, nl);
    float* geom = (float*)malloc(16 * (f4 ? f4 : 1));
    float* ptex = (float*)malloc(32 * (size_t)(np ? np : 1));
    if (!geom || !ptex) { free(geom); free(ptex); return 0; }
    wprep_build((const uint8_t*)spheres, ns, (const uint8_t*)planes, np, (const uint8_t*)lights, nl, geom, ptex);
    const float *gs = geom, *gp = geom + 4 * (size_t)ns, *gl = geom + 4 * (size_t)ns + 8 * (size_t)np;
    for (uint32_t k = 0; k < n; k++) {
        const ref_v3 p = ref_ld(probes[k].point);
        const float reach = probes[k].reach;
        const uint32_t skip = ignore ? ignore[k] : CLW_ID_NONE;
        s->best = INFINITY; s->best_id = CLW_ID_NONE; s->any = 0; s->L.count = 0u; s->L.K = s->K;
        if (flags & CLW_CAST_SPHERES)
            for (uint32_t i = 0; i < ns; i++) {
                const float* w = gs + 4 * (size_t)i;
                if (i == skip || ((flags & CLW_CAST_OPAQUE) && sign_bit(w[3]))) continue;
                const float d = ref_near_sphere(ref_sub(p, ref_ld(w)), w[3]);
                if (ref_near_candidate(d, reach)) take(s, d, i);
            }
        if (flags & CLW_CAST_PLANES)
            for (uint32_t i = 0; i < np; i++) {
                if (((1u << 30) | i) == skip) continue;
                const float d = fabsf(ref_near_plane_s(p, ref_ld(gp + 8 * (size_t)i), ref_ld(gp + 8 * (size_t)i + 4)));
                if (ref_near_candidate(d, reach)) take(s, d, (1u << 30) | i);
            }
        if (flags & CLW_CAST_LIGHTS)
            for (uint32_t i = 0; i < nl; i++) {
                if (((2u << 30) | i) == skip) continue;
                const float* w = gl + 8 * (size_t)i;
                const float d = ref_near_sphere(ref_sub(p, ref_ld(w)), w[3]);
                if (ref_near_candidate(d, reach)) take(s, d, (2u << 30) | i);
            }
        if (s->within) s->within[k] = (uint8_t)s->any;
        if (s->hits) {
            clw_hit* h = s->hits + k;
            h->t = s->best;
            h->id = s->best_id;
            for (int a = 0; a < 3; a++) { h->normal[a] = 0.0f; h->point[a] = 0.0f; }
            if (s->best_id != CLW_ID_NONE) {
                const uint32_t kind = s->best_id >> 30, index = s->best_id & 0x3FFFFFFFu;
                if (kind == 1u) {
                    const ref_v3 nrm = ref_ld(gp + 8 * (size_t)index);
                    ref_st(h->normal, nrm);
                    ref_st(h->point, ref_near_plane_point(p, nrm, ref_near_plane_s(p, nrm, ref_ld(gp + 8 * (size_t)index + 4))));
                } else {
                    const float* w = kind == 0u ? gs + 4 * (size_t)index : gl + 8 * (size_t)index;
                    ref_v3 nrm, point;
                    ref_near_sphere_point(p, ref_ld(w), w[3], &nrm, &point);
                    ref_st(h->normal, nrm);
                    ref_st(h->point, point);
                }
            }
        }
        for (uint32_t j = 0; j < s->K; j++) {      /* planar, layer-major */
            s->d_out[(size_t)j * n + k] = j < s->L.count ? s->L.e[j].t : INFINITY;
            s->id_out[(size_t)j * n + k] = j < s->L.count ? s->L.e[j].id : CLW_ID_NONE;
        }
    }
    free(geom);
    free(ptex);
    return 1;
}

int clw_host_nearest_surface(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                             const void* planes, uint32_t np, const void* lights, uint32_t nl, clw_hit* out) {
    if (!out) return 0;
    near_sink s = {0};
    s.hits = out;
    return near_enumerate(probes, ignore, n, flags, spheres, ns, planes, np, lights, nl, &s);
}

int clw_host_within_reach(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                          const void* planes, uint32_t np, const void* lights, uint32_t nl, uint8_t* within) {
    if (!within) return 0;
    near_sink s = {0};
    s.within = within;
    return near_enumerate(probes, ignore, n, flags, spheres, ns, planes, np, lights, nl, &s);
}

int clw_host_near_surfaces(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                           const void* planes, uint32_t np, const void* lights, uint32_t nl, uint32_t K, float* d, uint32_t* id) {
    if (!wt_near_list_check(n, flags, K) || !d || !id) return 0;
    near_sink s = {0};
    s.d_out = d; s.id_out = id; s.K = K;
    return near_enumerate(probes, ignore, n, flags, spheres, ns, planes, np, lights, nl, &s);
}
