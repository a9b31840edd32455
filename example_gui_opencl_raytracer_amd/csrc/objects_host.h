/* objects_host.h -- the visible-object table's definition on the host (include/hip_wrap_ext.h: clw_object_stat, clw_host_object_stats) and
 * the one check of its arguments, with the one clipping of its rectangle, that the host model and the shim (clw_ext_object_stats,
 * clw_ext_unit_object_stats) share. */
#ifndef OBJECTS_HOST_H
#define OBJECTS_HOST_H
#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WT_OBJ_MAX_SLOTS (1u << 24)      /* counts[0] + counts[1] + counts[2] + 1 slots at most */
#define WT_OBJ_MAX_PIXELS (1u << 30)     /* width * rows fits 30 bits */

/* 1 = arguments the table accepts, 0 = refused: a NULL `ids`, `counts` or `summary`, a width or rows of zero, a rectangle (when there is one)
 * of zero width or height, more than 2^24 slots, width * rows not fitting 30 bits, a last row beyond 2^32 - 1 (its y would not fit a record) */
int wt_objects_check(const void* ids, uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect, const uint32_t counts[3],
                     const void* summary);

/* The rectangle (NULL = the whole frame) clipped, in 64-bit arithmetic, to the columns 0 .. width - 1 and the rows first_row .. first_row +
 * rows - 1 of a checked range -> clip = {first column, first row OF THE RANGE (local), columns, rows}; 0 (and clip = 0, 0, 0, 0) when the
 * rectangle misses the range. */
int wt_objects_clip(uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect, uint32_t clip[4]);

#ifdef __cplusplus
}
#endif
#endif /* OBJECTS_HOST_H */
