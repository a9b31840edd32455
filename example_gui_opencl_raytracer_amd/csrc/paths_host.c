/* paths_host.c -- THE definition of the path queries (include/hip_wrap_ext.h: clw_host_cast_paths): the device pass (wt_cast_paths:
 * whitted_paths.inc) is held to it bit for bit.  Written for reading, not for speed.  A segment's hit is not defined again here: segment k of
 * every path is clw_host_cast_rays (cast_host.c) of the n current rays, written straight into layer k of the output -- a path that has ended
 * keeps a ray that meets nothing, so its later layers receive that query's miss record.  What is defined here is what becomes of a hit: whether
 * the path goes on (ref_path_stops), and the reference's outgoing ray (ref_bounce: raytracing.cl:139-179, primitives.cl:127-144) -- both in
 * ref_tests.h, the one text the device pass is compiled from too.  Built with -ffp-contract=off: every float32 operation is rounded once. */
#include "paths_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cast_host.h"
#include "ref_tests.h"

int wt_paths_check(uint32_t n, uint32_t flags, uint32_t bounces) {
    if (flags & ~(WT_PATHS_CAST_FLAGS | CLW_PATH_TRANSMIT | CLW_PATH_ALL_SURFACES)) return 0;
    return wt_cast_check(n, flags & WT_PATHS_CAST_FLAGS) && bounces >= 1u && bounces <= (uint32_t)WT_PATHS_MAX;
}

static ref_material material_of(uint32_t id, const void* spheres, const void* planes) {
    ref_material m;
    const uint8_t* rec = (const uint8_t*)((id >> 30) == 0u ? spheres : planes) + 96 * (size_t)(id & 0x3FFFFFFFu);
    memcpy(&m, rec + 64, sizeof m);
    return m;
}

int clw_host_cast_paths(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t bounces, const void* spheres, uint32_t ns, const void* planes,
                        uint32_t np, const void* lights, uint32_t nl, clw_hit* hits, uint8_t* status, clw_ray* next) {
    if (!wt_paths_check(n, flags, bounces) || !rays || !hits || !status || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights))
        return 0;
    clw_ray* cur = (clw_ray*)malloc((size_t)n * sizeof(clw_ray));      /* the ray of every path's segment under way */
    float* n1 = (float*)malloc((size_t)n * sizeof(float));
    uint8_t* ended = (uint8_t*)calloc(n, 1);
    if (!cur || !n1 || !ended) { free(cur); free(n1); free(ended); return 0; }
    memcpy(cur, rays, (size_t)n * sizeof(clw_ray));
    for (uint32_t i = 0; i < n; i++) n1[i] = REF_DEFAULT_N;
    int ok = 1;
    for (uint32_t k = 0; k < bounces && ok; k++) {
        clw_hit* layer = hits + (size_t)k * n;
        ok = clw_host_cast_rays(cur, n, flags & WT_PATHS_CAST_FLAGS, spheres, ns, planes, np, lights, nl, layer);      /* (refuses at k = 0 or never) */
        for (uint32_t i = 0; i < n && ok; i++) {
            if (ended[i]) continue;
            const clw_hit* h = layer + i;
            if (h->id == CLW_ID_NONE) {      /* a miss: cur[i] stays the ray that missed */
                status[i] = (uint8_t)(k | CLW_PATH_REASON_MISSED << 4);
                ended[i] = 1;
                continue;
            }
            const ref_v3 nrm = ref_ld(h->normal), p = ref_hit_offset(ref_ld(h->point), nrm);      /* the point shading uses */
            ref_v3 o = p, d = ref_mk(0.0f, 0.0f, 0.0f);
            int stops = (h->id >> 30) == 2u;      /* a light */
            ref_material m = {0u, 0u, 0.0f, 0.0f};
            if (!stops) {
                m = material_of(h->id, spheres, planes);
                stops = ref_path_stops(&m, (flags & CLW_PATH_ALL_SURFACES) != 0u);
            }
            if (!stops) ref_bounce(p, nrm, ref_ld(cur[i].dir), &m, (flags & CLW_PATH_TRANSMIT) != 0u, &n1[i], &o, &d);
            ref_st(cur[i].origin, o);
            ref_st(cur[i].dir, d);
            cur[i].ignore = CLW_ID_NONE;      /* (tmax stays the caller's) */
            if (stops) {
                status[i] = (uint8_t)((k + 1u) | CLW_PATH_REASON_ENDED << 4);
                ended[i] = 1;
                continue;
            }
            if (k + 1u == bounces) status[i] = (uint8_t)(bounces | CLW_PATH_REASON_BOUNCES << 4);
        }
    }
    if (ok && next) memcpy(next, cur, (size_t)n * sizeof(clw_ray));
    free(cur);
    free(n1);
    free(ended);
    return ok;
}
