/* paths_host.h -- the path queries' definition on the host (include/hip_wrap_ext.h: clw_host_cast_paths) and the one check of their arguments
 * that the host model and the shim (clw_ext_cast_paths, clw_ext_cast_paths_device, clw_ext_pick_path) share. */
#ifndef PATHS_HOST_H
#define PATHS_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { WT_PATHS_MAX = 8 };      /* the largest number of segments (CLW_PATH_MAX_BOUNCES) */
#define WT_PATHS_CAST_FLAGS (CLW_CAST_KINDS | CLW_CAST_OPAQUE)      /* the bits of a path query's flags that are the ray queries' */

/* 1 = a ray count, a flag word and a segment count the path query accepts, 0 = refused: a flag bit beside the ray queries' and the two
 * CLW_PATH_* ones, what wt_cast_check (cast_host.h) refuses for the ray queries' bits, bounces == 0, bounces > WT_PATHS_MAX */
int wt_paths_check(uint32_t n, uint32_t flags, uint32_t bounces);

#ifdef __cplusplus
}
#endif
#endif /* PATHS_HOST_H */
