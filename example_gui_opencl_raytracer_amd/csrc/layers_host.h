/* layers_host.h -- the layered ray queries' definition on the host (include/hip_wrap_ext.h: clw_layer, clw_host_cast_layers,
 * clw_host_camera_rays) and the one check of their arguments that the host model and the shim (clw_ext_cast_layers,
 * clw_ext_cast_layers_device, clw_ext_render_layers, clw_ext_pick_layers) share. */
#ifndef LAYERS_HOST_H
#define LAYERS_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { WT_LAYERS_MAX = 8 };      /* the largest K: the capacity of the larger of the two compiled kernels (whitted_layers.inc) */

/* 1 = a ray count, a flag word and a layer count the layered query accepts, 0 = refused: what wt_cast_check (cast_host.h) refuses, K == 0,
 * K > WT_LAYERS_MAX */
int wt_layers_check(uint32_t n, uint32_t flags, uint32_t K);

#ifdef __cplusplus
}
#endif
#endif /* LAYERS_HOST_H */
