/*
 * projection_host.h -- the camera models beside the pinhole (include/hip_wrap_ext.h: clw_projection): the terms a projection is resolved
 * into once per (camera, frame, projection), shared by the host definition (projection_host.c: clw_host_projection_rays), the shim and the
 * kernels (whitted_projection.inc: wt_proj_ray), which take the struct as a by-value argument of their own.  Plain C, no HIP.
 */
#ifndef PROJECTION_HOST_H
#define PROJECTION_HOST_H
#include <stdint.h>

#include "../../include/hip_wrap_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wt_projection {
    uint32_t model;                     /* CLW_PROJ_*; CLW_PROJ_PERSPECTIVE = the pinhole: nothing below is read */
    uint32_t width, height;             /* the frame the tables are for */
    uint32_t reserved;
    float origin[3];                    /* the camera origin */
    float dir[3];                       /* ORTHO: the unit axis, the direction of every ray; EQUIRECT: the unit axis */
    float corner[3], right[3], up[3];   /* ORTHO: the image plane, as wt_primary_dir_xy reads it (rescaled when ortho_width > 0) */
    float w_factor, h_factor;
    const float* col;                   /* EQUIRECT: width float4 { sin(theta) r + cos(theta) a, 0 }; the host resolves it to NULL */
    const float* row;                   /* EQUIRECT: height float4 { cos(phi), sin(phi) u } */
} wt_projection;

/* camera + projection -> the scalar terms (col = row = NULL); 0 = refused (what clw_host_projection_rays refuses), model 0 included */
int wt_projection_terms(const clw_camera* cam, const clw_projection* proj, wt_projection* out);
/* the ray of pixel (x, y): the float operations wt_proj_ray performs on the device, in the same order, without contraction */
void wt_projection_ray(const wt_projection* T, const float* col, const float* row, uint32_t x, uint32_t y, float o[3], float d[3]);

#ifdef __cplusplus
}
#endif
#endif
