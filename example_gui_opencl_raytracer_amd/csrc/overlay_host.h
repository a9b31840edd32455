/* overlay_host.h -- the selection overlay's definition on the host (include/hip_wrap_ext.h: clw_overlay, clw_host_overlay) and the one
 * check of a style and a selection that the host model and the shim (clw_ext_render_overlay, clw_ext_unit_overlay) share. */
#ifndef OVERLAY_HOST_H
#define OVERLAY_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WT_OV_MAX_RADIUS 4u
#define WT_OV_MAX_SEL 64u

/* 1 = a style and a selection the overlay accepts, 0 = refused: a NULL style, unknown flag bits, no flag at all, OUTLINE with a radius outside
 * 1..4, FILL with alpha > 256, more than 64 ids, ids without their array */
int wt_overlay_check(const clw_overlay* style, const uint32_t* sel, uint32_t count);

#ifdef __cplusplus
}
#endif
#endif /* OVERLAY_HOST_H */
