/* cast_host.h -- the ray queries' definition on the host (include/hip_wrap_ext.h: clw_ray, clw_hit, clw_host_cast_rays,
 * clw_host_occluded_rays) and the one check of their arguments that the host model and the shim (clw_ext_cast_rays, clw_ext_occluded_rays,
 * clw_ext_cast_rays_device) share. */
#ifndef CAST_HOST_H
#define CAST_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 = a ray count and a flag word the queries accept, 0 = refused: n == 0 or n >= 1 << 30, a flag bit outside CLW_CAST_KINDS |
 * CLW_CAST_OPAQUE, no kind bit set */
int wt_cast_check(uint32_t n, uint32_t flags);

/* The one copy of the queries' per-ray rule (cast_host.c), which the nearest, the any-hit and the layered definition (layers_host.c) share:
 * checks the arguments (wt_cast_check, null pointers: 0 = refused, nothing called), builds the words the device reads, and for every ray, in
 * order, calls `ray_begin` (the visitor empties its per-ray state there), then `take` for each candidate -- a primitive of a kind `flags`
 * names, not the ray's `ignore`, not transparent under CLW_CAST_OPAQUE, hit, at t <= tmax -- in scan order (spheres, planes, lights,
 * ascending index; id = kind << 30 | index), then `ray_done` with the ray's index.  `g` holds the words for as long as the call lasts: a nearest hit's point and normal are computed from them. */
typedef struct { const float* spheres; const float* planes; const float* lights; } wt_cast_geom;      /* 4, 8 and 8 floats per primitive */
typedef struct {
    void (*ray_begin)(void* ctx);
    void (*take)(void* ctx, float t, uint32_t id);
    void (*ray_done)(void* ctx, uint32_t k, const clw_ray* ray, const wt_cast_geom* g);
    void* ctx;
} wt_cast_visitor;
__attribute__((visibility("hidden")))      /* internal: shared by two objects of the library, not exported */
int wt_cast_enumerate(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                      const void* lights, uint32_t nl, const wt_cast_visitor* v);

#ifdef __cplusplus
}
#endif
#endif /* CAST_HOST_H */
