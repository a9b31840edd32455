/*
 * projection_host.c -- THE definition of the rays of the camera models beside the pinhole (include/hip_wrap_ext.h: clw_projection,
 * clw_host_projection_rays), and the host half of what the device needs to reproduce them bit for bit (projection_host.h).
 *
 * A projection is resolved ONCE per (camera, frame, projection) into scalar terms and, for the panorama, two small tables; everything
 * transcendental or double happens there, on the host.  The ray of a pixel is then a handful of float operations, one rounding each, no
 * contraction, IEEE square root and divide -- wt_projection_ray here, wt_proj_ray in csrc/whitted_projection.inc: each with its own table
 * addressing around the one text of the arithmetic (ref_tests.h), so host and device agree to the bit.  Built with -ffp-contract=off, like
 * host_camera.c.
 */
#include "projection_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ref_tests.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

static int finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
static int zero3(const float* v) { return v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f; }

/* the view direction: `axis`, or -- all zero -- the direction from the camera origin to the centre of its image plane (im_corner is
 * relative to the origin; the centre in double, rounded to float); normalised once in float */
static int unit_axis(const clw_camera* cam, const clw_projection* p, float a[3]) {
    float v[3] = {p->axis[0], p->axis[1], p->axis[2]};
    if (!finite3(v)) return 0;
    if (zero3(v)) {
        double c2 = 0.0, extent = 0.0;
        for (int k = 0; k < 3; k++) {
            const double rw = (double)cam->right[k] * ((double)cam->w_factor * cam->width / 2), uh = (double)cam->up[k] * ((double)cam->h_factor * cam->height / 2);
            const double c = (double)cam->im_corner[k] + rw - uh;
            v[k] = (float)c;
            c2 += c * c; extent += rw * rw + uh * uh;
        }
        /* a plane centred on the origin has no centre direction; what float32 rounding leaves of one (below 1e-6 of the plane's half
         * diagonal) is noise, not a direction */
        if (!(c2 > 1e-12 * extent)) return 0;
    }
    if (!finite3(v) || zero3(v)) return 0;
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(len > 0.0f) || !isfinite(len)) return 0;
    for (int k = 0; k < 3; k++) a[k] = v[k] / len;
    return finite3(a);
}

static int projection_ok(const clw_camera* cam, const clw_projection* p) {
    if (!cam || !p || cam->width == 0u || cam->height == 0u) return 0;
    if (p->model > CLW_PROJ_EQUIRECT || p->reserved != 0u) return 0;
    if (!isfinite(p->ortho_width) || p->ortho_width < 0.0f) return 0;
    if (!isfinite(p->h_span) || p->h_span < 0.0f || p->h_span > 360.0f) return 0;
    if (!isfinite(p->v_span) || p->v_span < 0.0f || p->v_span > 180.0f) return 0;
    if (!finite3(cam->im_corner) || !finite3(cam->origin) || !finite3(cam->up) || !finite3(cam->right) || !isfinite(cam->w_factor) ||
        !isfinite(cam->h_factor))
        return 0;
    return finite3(p->axis);
}

int wt_projection_terms(const clw_camera* cam, const clw_projection* p, wt_projection* T) {
    if (!T || !projection_ok(cam, p)) return 0;
    memset(T, 0, sizeof *T);
    T->model = p->model; T->width = cam->width; T->height = cam->height;
    memcpy(T->origin, cam->origin, 12); memcpy(T->corner, cam->im_corner, 12); memcpy(T->right, cam->right, 12); memcpy(T->up, cam->up, 12);
    T->w_factor = cam->w_factor; T->h_factor = cam->h_factor;
    if (p->model == CLW_PROJ_PERSPECTIVE) return 1;
    if (!unit_axis(cam, p, T->dir)) return 0;
    if (p->model == CLW_PROJ_ORTHO && p->ortho_width > 0.0f) {
        /* the frame's width spans ortho_width world units about the same centre: both factors times s, the corner moved (double, stored to float) */
        const double W = cam->width, H = cam->height;
        double r2 = 0.0, c[3];
        for (int k = 0; k < 3; k++) {
            r2 += (double)cam->right[k] * cam->right[k];
            c[k] = (double)cam->im_corner[k] + (double)cam->right[k] * ((double)cam->w_factor * W / 2) - (double)cam->up[k] * ((double)cam->h_factor * H / 2);
        }
        const double span = sqrt(r2) * fabs((double)cam->w_factor) * W;
        if (!(span > 0.0) || !isfinite(span)) return 0;
        const double s = (double)p->ortho_width / span;
        T->w_factor = (float)((double)cam->w_factor * s);
        T->h_factor = (float)((double)cam->h_factor * s);
        for (int k = 0; k < 3; k++)
            T->corner[k] = (float)(c[k] - (double)cam->right[k] * ((double)T->w_factor * W / 2) + (double)cam->up[k] * ((double)T->h_factor * H / 2));
        if (!finite3(T->corner) || !isfinite(T->w_factor) || !isfinite(T->h_factor)) return 0;
    }
    return 1;
}

/* EQUIRECT: the camera's right and up made orthonormal to the unit axis (Gram-Schmidt, double); 0 = one of them is parallel to it */
static int panorama_frame(const clw_camera* cam, const float axis[3], double a[3], double r[3], double u[3]) {
    /* (what is left of a vector after the projection must stand above float32 rounding: 1e-5 of its length) */
    double ra = 0.0, ua = 0.0, ur = 0.0, len = 0.0, rr = 0.0, uu = 0.0;
    for (int k = 0; k < 3; k++) {
        a[k] = axis[k]; ra += (double)cam->right[k] * a[k]; ua += (double)cam->up[k] * a[k];
        rr += (double)cam->right[k] * cam->right[k]; uu += (double)cam->up[k] * cam->up[k];
    }
    for (int k = 0; k < 3; k++) { r[k] = (double)cam->right[k] - ra * a[k]; len += r[k] * r[k]; }
    len = sqrt(len);
    if (!(len > 1e-5 * sqrt(rr)) || !isfinite(len)) return 0;
    for (int k = 0; k < 3; k++) { r[k] /= len; ur += (double)cam->up[k] * r[k]; }
    len = 0.0;
    for (int k = 0; k < 3; k++) { u[k] = (double)cam->up[k] - ua * a[k] - ur * r[k]; len += u[k] * u[k]; }
    len = sqrt(len);
    if (!(len > 1e-5 * sqrt(uu)) || !isfinite(len)) return 0;
    for (int k = 0; k < 3; k++) u[k] /= len;
    return 1;
}

int clw_host_projection_tables(const clw_camera* cam, const clw_projection* proj, float* col4, float* row4) {
    wt_projection T;
    double a[3], r[3], u[3];
    if (!col4 || !row4 || !wt_projection_terms(cam, proj, &T) || T.model != CLW_PROJ_EQUIRECT) return 0;
    if (!panorama_frame(cam, T.dir, a, r, u)) return 0;
    const double hs = (proj->h_span == 0.0f ? 360.0 : (double)proj->h_span) * (M_PI / 180.0);
    const double vs = (proj->v_span == 0.0f ? 180.0 : (double)proj->v_span) * (M_PI / 180.0);
    const int64_t W = cam->width, H = cam->height;
    /* pixel centres: theta(x) = ((x + 1/2) / W - 1/2) h_span, phi(y) = (1/2 - (y + 1/2) / H) v_span, written over the common denominator so
     * that column x and column W - 1 - x (row y and row H - 1 - y) get angles that are each other's negative EXACTLY */
    for (int64_t x = 0; x < W; x++) {
        const double th = (double)(2 * x + 1 - W) / (double)(2 * W) * hs, s = sin(th), c = cos(th);
        for (int k = 0; k < 3; k++) col4[4 * x + k] = (float)(s * r[k] + c * a[k]);
        col4[4 * x + 3] = 0.0f;
    }
    for (int64_t y = 0; y < H; y++) {
        const double ph = (double)(H - 1 - 2 * y) / (double)(2 * H) * vs, s = sin(ph);
        row4[4 * y] = (float)cos(ph);
        for (int k = 0; k < 3; k++) row4[4 * y + 1 + k] = (float)(s * u[k]);
    }
    return 1;
}

void wt_projection_ray(const wt_projection* T, const float* col, const float* row, uint32_t x, uint32_t y, float o[3], float d[3]) {
    ref_v3 v;
    if (T->model == CLW_PROJ_EQUIRECT) {
        const float* r = row + 4 * (size_t)y;
        v = ref_madd(ref_ld(col + 4 * (size_t)x), r[0], ref_ld(r + 1));
    } else {
        /* the image-plane vector of the pinhole raygen (raygen.cl:13-17), the operations of wt_primary_dir_xy before its sqrtf, in that order */
        v = ref_image_plane(ref_ld(T->corner), ref_ld(T->right), ref_ld(T->up), T->w_factor, T->h_factor, x, y);
        if (T->model == CLW_PROJ_ORTHO) {      /* parallel rays from the image plane: it is the near plane */
            ref_st(o, ref_add(ref_ld(T->origin), v));
            ref_st(d, ref_ld(T->dir));
            return;
        }
    }
    ref_st(o, ref_ld(T->origin));
    ref_st(d, ref_normalize(v));
}

int clw_host_projection_rays(const clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end, float* rays16) {
    wt_projection T;
    if (!rays16 || !wt_projection_terms(cam, proj, &T)) return 0;
    const uint64_t W = cam->width, total = W * cam->height;
    if (id_begin > id_end || id_end > total) return 0;
    float *col = NULL, *row = NULL;
    if (T.model == CLW_PROJ_EQUIRECT) {
        col = (float*)malloc(16 * (size_t)cam->width);
        row = (float*)malloc(16 * (size_t)cam->height);
        if (!col || !row || !clw_host_projection_tables(cam, proj, col, row)) { free(col); free(row); return 0; }
    }
    for (uint64_t id = id_begin; id < id_end; id++) {
        float* rec = rays16 + 16 * (size_t)(id - id_begin);
        memset(rec, 0, 64);      /* {origin, 0, dir, 0, rgb = 0, depth = 0 + pad} */
        wt_projection_ray(&T, col, row, (uint32_t)(id % W), (uint32_t)(id / W), rec, rec + 4);
    }
    free(col); free(row);
    return 1;
}

int clw_host_ortho_camera(const float origin[3], const float look[3], float view_width, uint32_t width, uint32_t height, clw_camera* cam,
                          clw_projection* proj) {
    if (!origin || !look || !cam || !proj || width == 0u || height == 0u) return 0;
    if (!finite3(origin) || !finite3(look) || zero3(look) || !isfinite(view_width) || !(view_width > 0.0f)) return 0;
    /* right and up as clw_host_perspective builds them: dir = look / |look| (double sqrt), right = (0, 1, 0) x forward, up = forward x right */
    const float inv = 1 / sqrt((double)look[0] * look[0] + (double)look[1] * look[1] + (double)look[2] * look[2]);
    const float dir[3] = {look[0] * inv, look[1] * inv, look[2] * inv};
    const float fwd[3] = {dir[0] * -1.0f, dir[1] * -1.0f, dir[2] * -1.0f};
    const float right[3] = {1.0f * fwd[2] - 0.0f * fwd[1], 0.0f * fwd[0] - 0.0f * fwd[2], 0.0f * fwd[1] - 1.0f * fwd[0]};
    const float up[3] = {fwd[1] * right[2] - fwd[2] * right[1], fwd[2] * right[0] - fwd[0] * right[2], fwd[0] * right[1] - fwd[1] * right[0]};
    if (!finite3(dir) || zero3(right) || zero3(up)) return 0;      /* look along +-Y: no `right` (cpu_ray.c:58-63 rejects +Y) */
    memset(cam, 0, sizeof *cam);
    memset(proj, 0, sizeof *proj);
    cam->width = width; cam->height = height;
    cam->w_factor = view_width / width;
    cam->h_factor = cam->w_factor;                                 /* square pixels */
    const float image_w = view_width, image_h = cam->h_factor * height;
    for (int k = 0; k < 3; k++) {
        cam->origin[k] = origin[k]; cam->right[k] = right[k]; cam->up[k] = up[k];
        cam->im_corner[k] = 0.0f - right[k] * image_w / 2 + up[k] * image_h / 2;      /* the image plane passes through the origin */
        proj->axis[k] = dir[k];
    }
    proj->model = CLW_PROJ_ORTHO;
    /* `right` is not unit when `look` leaves the horizontal (as in clw_host_perspective): the projection rescales the plane so that the
     * frame's width spans view_width whatever its length */
    proj->ortho_width = view_width;
    wt_projection T;
    return wt_projection_terms(cam, proj, &T);
}
