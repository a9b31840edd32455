/* paths_host.c -- THE definition of the path queries (include/hip_wrap_ext.h: clw_host_cast_paths): the device pass (wt_cast_paths:
 * whitted_paths.inc) is held to it bit for bit.  Written for reading, not for speed.  A segment's hit is not defined again here: segment k of
 * every path is clw_host_cast_rays (cast_host.c) of the n current rays, written straight into layer k of the output -- a path that has ended
 * keeps a ray that meets nothing, so its later layers receive that query's miss record.  What is defined here is what becomes of a hit: whether
 * the path goes on, and the reference's outgoing ray (raytracing.cl:139-179, primitives.cl:127-144).  Built with -ffp-contract=off: every
 * float32 operation below is rounded once. */
#include "paths_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cast_host.h"
#include "ref_tests.h"

#define EPSILON 0.001f         /* primitives.cl:5 */
#define DEFAULT_N 1.0f         /* raytracing.cl:7 */

int wt_paths_check(uint32_t n, uint32_t flags, uint32_t bounces) {
    if (flags & ~(WT_PATHS_CAST_FLAGS | CLW_PATH_TRANSMIT | CLW_PATH_ALL_SURFACES)) return 0;
    return wt_cast_check(n, flags & WT_PATHS_CAST_FLAGS) && bounces >= 1u && bounces <= (uint32_t)WT_PATHS_MAX;
}

/* the four words of a 96-byte sphere or plane record that decide where a path goes: byte 64 = offset 32 of its material */
typedef struct { uint32_t transperent, dielectric; float n, reflectivity; } path_material;

static path_material material_of(uint32_t id, const void* spheres, const void* planes) {
    path_material m;
    const uint8_t* rec = (const uint8_t*)((id >> 30) == 0u ? spheres : planes) + 96 * (size_t)(id & 0x3FFFFFFFu);
    memcpy(&m, rec + 64, sizeof m);
    return m;
}

/* primitives.cl:127-130 */
static void reflect(const float i[3], const float n[3], float out[3]) {
    const float cosI = -dot3(n, i);
    for (int a = 0; a < 3; a++) out[a] = i[a] + n[a] * (2 * cosI);
}

/* primitives.cl:132-144: a NaN vector on total internal reflection; `i` is taken for unit */
static void refract(float n1, float n2, const float i[3], const float nrm[3], float out[3]) {
    const float n = n1 / n2;
    const float cosI = -dot3(nrm, i);
    const float sinT2 = n * n * (1.0f - cosI * cosI);
    if (sinT2 > 1.0f) { out[0] = out[1] = out[2] = NAN; return; }
    const float cosT = sqrtf(1.0f - sinT2);
    for (int a = 0; a < 3; a++) out[a] = i[a] * n + nrm[a] * (n * cosI - cosT);
}

/* The ray that leaves hit `h` of ray `r` on a surface of material `m`, into `r` itself; *n1 = the path's refractive index, updated.
 * raytracing.cl:139-179 without the weights: the reflected ray, or with CLW_PATH_TRANSMIT through a transparent surface the refracted one. */
static void bounce(clw_ray* r, const clw_hit* h, const path_material* m, uint32_t flags, float* n1) {
    float p[3], out[3];
    for (int a = 0; a < 3; a++) p[a] = h->point[a] + h->normal[a] * EPSILON;      /* the point shading uses (primitives.cl:339, 357) */
    reflect(r->dir, h->normal, out);
    if ((flags & CLW_PATH_TRANSMIT) && m->transperent) {
        const float n2 = (*n1 == DEFAULT_N) ? m->n : DEFAULT_N;
        float nrm[3], o[3], through[3];
        for (int a = 0; a < 3; a++) { nrm[a] = h->normal[a]; o[a] = p[a]; }
        if (*n1 < n2) { for (int a = 0; a < 3; a++) o[a] = p[a] - nrm[a] * (2 * EPSILON); }
        else { for (int a = 0; a < 3; a++) nrm[a] = nrm[a] * -1; }
        refract(*n1, n2, r->dir, nrm, through);
        if (!(through[0] != through[0])) {      /* (total internal reflection: the reflected ray from p, n1 as it was) */
            for (int a = 0; a < 3; a++) { p[a] = o[a]; out[a] = through[a]; }
            *n1 = n2;
        }
    }
    for (int a = 0; a < 3; a++) { r->origin[a] = p[a]; r->dir[a] = out[a]; }
    r->ignore = CLW_ID_NONE;      /* (tmax stays the caller's) */
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
    for (uint32_t i = 0; i < n; i++) n1[i] = DEFAULT_N;
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
            int stops = (h->id >> 30) == 2u;      /* a light */
            path_material m = {0u, 0u, 0.0f, 0.0f};
            if (!stops) {
                m = material_of(h->id, spheres, planes);
                stops = !(flags & CLW_PATH_ALL_SURFACES) && m.reflectivity == 0 && !m.dielectric && !m.transperent;
            }
            if (stops) {
                for (int a = 0; a < 3; a++) { cur[i].origin[a] = h->point[a] + h->normal[a] * EPSILON; cur[i].dir[a] = 0.0f; }
                cur[i].ignore = CLW_ID_NONE;
                status[i] = (uint8_t)((k + 1u) | CLW_PATH_REASON_ENDED << 4);
                ended[i] = 1;
                continue;
            }
            bounce(&cur[i], h, &m, flags, &n1[i]);
            if (k + 1u == bounces) status[i] = (uint8_t)(bounces | CLW_PATH_REASON_BOUNCES << 4);
        }
    }
    if (ok && next) memcpy(next, cur, (size_t)n * sizeof(clw_ray));
    free(cur);
    free(n1);
    free(ended);
    return ok;
}
