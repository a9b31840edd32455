/* near_host.h -- the proximity queries' definition on the host (include/hip_wrap_ext.h: clw_probe, clw_host_nearest_surface,
 * clw_host_within_reach, clw_host_near_surfaces) and the one check of their arguments that the host model and the shim (clw_ext_nearest_surface,
 * clw_ext_within_reach, clw_ext_near_surfaces, clw_ext_probe_device, clw_ext_near_surfaces_device) share. */
#ifndef NEAR_HOST_H
#define NEAR_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 = a probe count and a flag word the proximity queries accept, 0 = refused: exactly what wt_cast_check (cast_host.h) refuses */
int wt_near_check(uint32_t n, uint32_t flags);
/* ... and a list length: K == 0 and K > WT_LAYERS_MAX (layers_host.h) are refused too */
int wt_near_list_check(uint32_t n, uint32_t flags, uint32_t K);

#ifdef __cplusplus
}
#endif
#endif /* NEAR_HOST_H */
