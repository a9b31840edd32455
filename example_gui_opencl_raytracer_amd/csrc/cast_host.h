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

#ifdef __cplusplus
}
#endif
#endif /* CAST_HOST_H */
