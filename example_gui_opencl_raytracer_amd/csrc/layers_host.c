/* layers_host.c -- THE definition of the layered ray queries (include/hip_wrap_ext.h: clw_host_cast_layers, clw_host_camera_rays): the device
 * passes (wt_cast_layers, wt_camera_rays: whitted_layers.inc) are held to it bit for bit.  Written for reading, not for speed: every ray on its
 * own against every primitive that takes part, the rules in the header's order.  The two tests are those of cast_host.c, restated: the same
 * operations in the same order.  Built with -ffp-contract=off: every float32 operation below is rounded once. */
#include "layers_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cast_host.h"
#include "scene_prep.h"

int wt_layers_check(uint32_t n, uint32_t flags, uint32_t K) { return wt_cast_check(n, flags) && K >= 1u && K <= (uint32_t)WT_LAYERS_MAX; }

static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* cast_host.c's ref_sphere and ref_plane */
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

/* a ray's list: the K smallest keys (t, id) met so far, ascending; entries past `count` are not read */
typedef struct { clw_layer e[WT_LAYERS_MAX]; uint32_t count, K; } layer_list;

static int key_before(float t, uint32_t id, const clw_layer* e) { return t < e->t || (t == e->t && id < e->id); }

/* a candidate (hit && t <= tmax) of the ray: listed iff t < +inf; kept iff it is among the K smallest keys */
static void list_candidate(layer_list* L, float t, uint32_t id) {
    if (!(t < INFINITY)) return;
    uint32_t at = L->count;
    while (at > 0u && key_before(t, id, &L->e[at - 1u])) at--;
    if (at >= L->K) return;
    if (L->count < L->K) L->count++;
    for (uint32_t j = L->count - 1u; j > at; j--) L->e[j] = L->e[j - 1u];
    L->e[at].t = t;
    L->e[at].id = id;
}

int clw_host_cast_layers(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, const void* spheres, uint32_t ns, const void* planes,
                         uint32_t np, const void* lights, uint32_t nl, float* t_out, uint32_t* id_out) {
    if (!wt_layers_check(n, flags, K) || !rays || !t_out || !id_out || (ns > 0u && !spheres) || (np > 0u && !planes) || (nl > 0u && !lights)) return 0;
    /* the words the device reads (cast_host.c) */
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
        layer_list L;
        L.count = 0u; L.K = K;
        float t;
        if (flags & CLW_CAST_SPHERES)
            for (uint32_t i = 0; i < ns; i++) {
                const float* s = geom + 4 * (size_t)i;
                if (i == ignore || ((flags & CLW_CAST_OPAQUE) && sign_bit(s[3]))) continue;
                if (ref_sphere(o, d, s, &t) && t <= tmax) list_candidate(&L, t, i);
            }
        if (flags & CLW_CAST_PLANES)
            for (uint32_t i = 0; i < np; i++) {
                if (((1u << 30) | i) == ignore) continue;
                if (ref_plane(o, d, pl + 8 * (size_t)i, pl + 8 * (size_t)i + 4, &t) && t <= tmax) list_candidate(&L, t, (1u << 30) | i);
            }
        if (flags & CLW_CAST_LIGHTS)
            for (uint32_t i = 0; i < nl; i++) {
                if (((2u << 30) | i) == ignore) continue;
                if (ref_sphere(o, d, lg + 8 * (size_t)i, &t) && t <= tmax) list_candidate(&L, t, (2u << 30) | i);
            }
        for (uint32_t j = 0; j < K; j++) {      /* planar, layer-major */
            t_out[(size_t)j * n + k] = j < L.count ? L.e[j].t : INFINITY;
            id_out[(size_t)j * n + k] = j < L.count ? L.e[j].id : CLW_ID_NONE;
        }
    }
    free(geom);
    free(ptex);
    return 1;
}

int clw_host_camera_rays(const struct clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end, clw_ray* out) {
    if (!out || id_begin > id_end) return 0;
    const uint64_t count = id_end - id_begin;
    if (count > ((size_t)-1) / 64u) return 0;
    float* rec = (float*)malloc(64 * (size_t)(count ? count : 1));      /* the 64-byte records {origin, 0, dir, 0, 0 ...} */
    if (!rec) return 0;
    if (!clw_host_projection_rays(cam, proj, id_begin, id_end, rec)) { free(rec); return 0; }
    for (uint64_t k = 0; k < count; k++) {
        const float* r = rec + 16 * (size_t)k;
        clw_ray* q = out + k;
        for (int a = 0; a < 3; a++) { q->origin[a] = r[a]; q->dir[a] = r[4 + a]; }
        q->tmax = INFINITY;
        q->ignore = CLW_ID_NONE;
    }
    free(rec);
    return 1;
}
