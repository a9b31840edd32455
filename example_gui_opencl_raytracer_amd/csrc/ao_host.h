/* ao_host.h -- the ambient occlusion pass's definition on the host (include/hip_wrap_ext.h: clw_ao, clw_host_ao_dirs, clw_host_ao_open,
 * clw_host_ao_resolve) and the one check of its parameters that the host model and the shim (clw_ext_render_ao, clw_ext_unit_ao_*) share. */
#ifndef AO_HOST_H
#define AO_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WT_AO_MAX_RAYS 32u
#define WT_AO_PATTERNS 16u

/* 1 = parameters the pass accepts, 0 = refused: a NULL pointer, unknown flag bits, rays outside 1..32, a radius that is NaN or <= 0,
 * strength > 256 */
int wt_ao_check(const clw_ao* ao);
/* 1 = a range the pass accepts: neither zero, width * rows below 2^30 */
int wt_ao_range_ok(uint32_t width, uint32_t rows);

#ifdef __cplusplus
}
#endif
#endif /* AO_HOST_H */
