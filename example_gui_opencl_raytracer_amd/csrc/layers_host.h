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

/* A query's list and its one rule (layers_host.c), which the layered ray query and the K-nearest proximity query (near_host.c) share: the K
 * smallest keys (t, id) met so far, ascending; entries past `count` are not read.  A candidate is listed iff t < +inf and kept iff it is among
 * the K smallest keys; an equal key keeps the earlier candidate. */
typedef struct { clw_layer e[WT_LAYERS_MAX]; uint32_t count, K; } wt_layer_list;
__attribute__((visibility("hidden")))      /* internal: shared by two objects of the library, not exported */
void wt_layers_candidate(wt_layer_list* L, float t, uint32_t id);

#ifdef __cplusplus
}
#endif
#endif /* LAYERS_HOST_H */
