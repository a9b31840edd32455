/* layers_host.c -- THE definition of the layered ray queries (include/hip_wrap_ext.h: clw_host_cast_layers, clw_host_camera_rays): the device
 * passes (wt_cast_layers, wt_camera_rays: whitted_layers.inc) are held to it bit for bit.  Written for reading, not for speed: every ray on its
 * own against every primitive that takes part, the rules in the header's order.  The per-ray rule -- which primitives are candidates, in which order -- is
 * cast_host.c's wt_cast_enumerate, the one copy; what is defined here is what becomes of a candidate.  Built with -ffp-contract=off: every float32 operation below is rounded once. */
#include "layers_host.h"

#include <math.h>
#include <stdlib.h>

#include "cast_host.h"

int wt_layers_check(uint32_t n, uint32_t flags, uint32_t K) { return wt_cast_check(n, flags) && K >= 1u && K <= (uint32_t)WT_LAYERS_MAX; }

static int key_before(float t, uint32_t id, const clw_layer* e) { return t < e->t || (t == e->t && id < e->id); }

/* a candidate (hit && t <= tmax) of the ray: listed iff t < +inf; kept iff it is among the K smallest keys */
void wt_layers_candidate(wt_layer_list* L, float t, uint32_t id) {
    if (!(t < INFINITY)) return;
    uint32_t at = L->count;
    while (at > 0u && key_before(t, id, &L->e[at - 1u])) at--;
    if (at >= L->K) return;
    if (L->count < L->K) L->count++;
    for (uint32_t j = L->count - 1u; j > at; j--) L->e[j] = L->e[j - 1u];
    L->e[at].t = t;
    L->e[at].id = id;
}

/* the visitor of cast_host.c's wt_cast_enumerate: the list of the ray under way, and where a finished one goes */
typedef struct { wt_layer_list L; float* t_out; uint32_t* id_out; uint32_t n; } layers_out;

static void layers_begin(void* ctx) { ((layers_out*)ctx)->L.count = 0u; }

static void layers_take(void* ctx, float t, uint32_t id) { wt_layers_candidate(&((layers_out*)ctx)->L, t, id); }

static void layers_done(void* ctx, uint32_t k, const clw_ray* ray, const wt_cast_geom* g) {
    layers_out* s = (layers_out*)ctx;
    (void)ray; (void)g;
    for (uint32_t j = 0; j < s->L.K; j++) {      /* planar, layer-major */
        s->t_out[(size_t)j * s->n + k] = j < s->L.count ? s->L.e[j].t : INFINITY;
        s->id_out[(size_t)j * s->n + k] = j < s->L.count ? s->L.e[j].id : CLW_ID_NONE;
    }
}

int clw_host_cast_layers(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, const void* spheres, uint32_t ns, const void* planes,
                         uint32_t np, const void* lights, uint32_t nl, float* t_out, uint32_t* id_out) {
    if (!wt_layers_check(n, flags, K) || !t_out || !id_out) return 0;
    layers_out s;
    s.L.count = 0u; s.L.K = K; s.t_out = t_out; s.id_out = id_out; s.n = n;
    const wt_cast_visitor v = {layers_begin, layers_take, layers_done, &s};
    return wt_cast_enumerate(rays, n, flags, spheres, ns, planes, np, lights, nl, &v);
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
