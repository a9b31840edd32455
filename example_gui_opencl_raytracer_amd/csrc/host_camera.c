/*
 * host_camera.c -- camera -> the six raygen scalars/vectors, for callers that do not link
 * the reference's src/cpu_ray.c (the bench driver, bench.py, the tests).
 *
 * Same results as the reference's rinit_camera + rgen_perspective
 * (reference src/cpu_ray.c:8-35, 42-106): the look direction is normalised with a
 * double-precision sqrt, the half-angle and tan() go through double and are stored to
 * float, `right`/`up` are not re-normalised, and the corner is
 * dir*focal - right*image_w/2 + up*image_h/2.  Built with -ffp-contract=off.
 */
#include "../../include/hip_wrap_ext.h"
#include <float.h>
#include <math.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

int clw_host_perspective(const float origin[3], const float look[3], float fov, float focal,
                         uint32_t width, uint32_t height, clw_camera* out) {
    /* rinit_camera: dir = look / |look| */
    float inv = 1 / sqrt(look[0] * look[0] + look[1] * look[1] + look[2] * look[2]);
    float dir[3] = {look[0] * inv, look[1] * inv, look[2] * inv};

    out->width = width;
    out->height = height;
    for (int k = 0; k < 3; k++) out->origin[k] = origin[k];

    int is_180 = fov - 180.0f <= FLT_EPSILON && fov - 180.0f >= 0;
    if (is_180 || fov <= FLT_EPSILON || (dir[0] == 0.0f && dir[1] == 1.0f && dir[2] == 0.0f)) return 0;

    float half_fov = (fov / 360.0f) * M_PI;
    float aspect = (float)height / (float)width;
    float fov_tan = tan(half_fov);
    float image_w = fov_tan * focal * 2;
    float image_h = aspect * image_w;
    out->w_factor = image_w / width;
    out->h_factor = image_h / height;

    float fwd[3] = {dir[0] * -1.0f, dir[1] * -1.0f, dir[2] * -1.0f};
    /* right = (0,1,0) x forward, up = forward x right, written out like the reference */
    float right[3] = {1.0f * fwd[2] - 0.0f * fwd[1], 0.0f * fwd[0] - 0.0f * fwd[2], 0.0f * fwd[1] - 1.0f * fwd[0]};
    float up[3] = {fwd[1] * right[2] - fwd[2] * right[1], fwd[2] * right[0] - fwd[0] * right[2],
                   fwd[0] * right[1] - fwd[1] * right[0]};
    for (int k = 0; k < 3; k++) {
        float centre = -fwd[k] * focal;
        out->right[k] = right[k];
        out->up[k] = up[k];
        out->im_corner[k] = centre - right[k] * image_w / 2 + up[k] * image_h / 2;
    }
    return 1;
}

/* ---- tables of n x n sample cameras (hip_wrap_ext.h: clw_ext_set_sample_cameras) ---------------------------------- */

static int sample_factor_lg(uint32_t n) { return n == 2 ? 1 : (n == 4 ? 2 : (n == 8 ? 3 : 0)); }

/* sample k = sy * n + sx -> lens cell / shutter slot j: k with its 2 log2 n bits reversed */
static uint32_t sample_slot(uint32_t k, int lg) {
    uint32_t j = 0;
    for (int b = 0; b < 2 * lg; b++) j |= ((k >> b) & 1u) << (2 * lg - 1 - b);
    return j;
}

int clw_host_lens_cameras(const clw_camera* base, float aperture, float focus, uint32_t n, clw_sample_camera* out) {
    const int lg = sample_factor_lg(n);
    if (!base || !out || !lg || !(aperture >= 0.0f) || !isfinite(aperture) || !(focus > 0.0f) || !isfinite(focus)) return 0;
    /* image-plane centre relative to the origin, its length (the focal distance), and q = focal / focus: double, q stored to float */
    double c2 = 0;
    for (int a = 0; a < 3; a++) {
        double c = (double)base->im_corner[a] + (double)base->right[a] * ((double)base->w_factor * base->width / 2)
                                              - (double)base->up[a] * ((double)base->h_factor * base->height / 2);
        c2 += c * c;
    }
    const double focal = sqrt(c2);
    if (!(focal > 0) || !isfinite(focal)) return 0;
    const float q = (float)(focal / (double)focus);
    if (!isfinite(q)) return 0;
    for (uint32_t k = 0; k < n * n; k++) {
        clw_sample_camera* o = out + k;
        memcpy(o->im_corner, base->im_corner, 12); memcpy(o->origin, base->origin, 12);
        memcpy(o->up, base->up, 12); memcpy(o->right, base->right, 12);
        if (aperture == 0.0f) continue;                /* the pinhole: the base camera, bit for bit */
        const uint32_t j = sample_slot(k, lg);
        /* centre of lens cell (j mod n, j div n) in [-1, 1]^2 -> unit disk, concentric map (Shirley & Chiu 1997): double, stored to float */
        const double a = (2.0 * (j % n) + 1.0) / n - 1.0, b = (2.0 * (j / n) + 1.0) / n - 1.0;
        double r, phi;
        if (fabs(a) > fabs(b)) { r = a; phi = (M_PI / 4) * (b / a); }
        else { r = b; phi = M_PI / 2 - (M_PI / 4) * (a / b); }      /* (n is even: no cell centre at 0, 0) */
        const float lx = (float)(r * cos(phi)), ly = (float)(r * sin(phi));
        const float ax = aperture * lx, ay = aperture * ly;
        for (int i = 0; i < 3; i++) {
            const float delta = base->right[i] * ax + base->up[i] * ay;
            o->origin[i] = base->origin[i] + delta;
            o->im_corner[i] = base->im_corner[i] - delta * q;
        }
    }
    return 1;
}

/* ---- progressive frame accumulation (hip_wrap_ext.h: clw_ext_set_accumulate) -------------------------------------- */

uint32_t clw_host_frame_seed(uint32_t f) { return f * 0x9E3779B1u; }      /* odd multiplier: a bijection mod 2^32, 0 for frame 0 */

/* the radical inverse of f in `base`: the usual digit loop, double */
static double radical_inverse(uint32_t f, uint32_t base) {
    const double inv = 1.0 / (double)base;
    double w = inv, r = 0.0;
    while (f) { r += (double)(f % base) * w; f /= base; w *= inv; }
    return r;
}

int clw_host_jitter_camera(const clw_camera* base, uint32_t f, uint32_t n, clw_camera* out) {
    if (!base || !out || (n != 1 && n != 2 && n != 4 && n != 8)) return 0;
    if (out != base) memcpy(out, base, sizeof *out);
    if (f == 0) return 1;                                /* frame 0: the base camera, byte for byte */
    /* the Halton point (2, 3) of the frame, centred: double, stored to float; everything after it in float32, one rounding per operation */
    const float jx = (float)(radical_inverse(f, 2) - 0.5), jy = (float)(radical_inverse(f, 3) - 0.5);
    const float cw = base->w_factor / (float)n, ch = base->h_factor / (float)n;      /* the cell of a sample */
    const float ax = cw * jx, ay = ch * jy;
    for (int i = 0; i < 3; i++) {
        const float rx = base->right[i] * ax, uy = base->up[i] * ay;
        const float c = base->im_corner[i] + rx;
        out->im_corner[i] = c - uy;
    }
    return 1;
}

static float shutter_mix(float a, float b, float t) { return a == b ? a : a + (b - a) * t; }

int clw_host_shutter_cameras(const clw_camera* open, const clw_camera* close, uint32_t n, clw_sample_camera* out) {
    const int lg = sample_factor_lg(n);
    if (!open || !close || !out || !lg) return 0;
    if (open->width != close->width || open->height != close->height ||
        memcmp(&open->w_factor, &close->w_factor, 4) || memcmp(&open->h_factor, &close->h_factor, 4)) return 0;
    for (uint32_t k = 0; k < n * n; k++) {
        const float t = ((float)sample_slot(k, lg) + 0.5f) / (float)(n * n);      /* exact */
        for (int i = 0; i < 3; i++) {
            out[k].im_corner[i] = shutter_mix(open->im_corner[i], close->im_corner[i], t);
            out[k].origin[i] = shutter_mix(open->origin[i], close->origin[i], t);
            out[k].up[i] = shutter_mix(open->up[i], close->up[i], t);
            out[k].right[i] = shutter_mix(open->right[i], close->right[i], t);
        }
    }
    return 1;
}

/* ---- moving spheres (hip_wrap_ext.h: clw_ext_set_sphere_motion) --------------------------------------------------- */

int clw_host_sample_times(uint32_t n, float* out) {
    const int lg = sample_factor_lg(n);
    if (!out || !lg) return 0;
    for (uint32_t k = 0; k < n * n; k++) out[k] = ((float)sample_slot(k, lg) + 0.5f) / (float)(n * n);      /* exact */
    return 1;
}

int clw_host_spheres_at(const void* rspheres, uint32_t ns, const float* disp, float t, void* out) {
    if (ns && (!rspheres || !disp || !out)) return 0;
    if (out != rspheres) memmove(out, rspheres, 96 * (size_t)ns);
    for (uint32_t i = 0; i < ns; i++) {
        float c[3];
        memcpy(c, (const unsigned char*)out + 96 * (size_t)i, 12);
        for (int a = 0; a < 3; a++) c[a] = fmaf(t, disp[3 * (size_t)i + a], c[a]);      /* one rounding, as the kernel's v_fma_f32 */
        memcpy((unsigned char*)out + 96 * (size_t)i, c, 12);
    }
    return 1;
}

/* ---- adaptive supersampling (hip_wrap_ext.h: clw_ext_set_adaptive) ------------------------------------------------- */

static uint32_t channel_contrast(uint32_t p, uint32_t q) {
    uint32_t c = 0;
    for (int s = 0; s < 24; s += 8) {
        const int d = (int)((p >> s) & 255u) - (int)((q >> s) & 255u);
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        if (a > c) c = a;
    }
    return c;
}

int clw_host_refine_mask(const uint32_t* xrgb, uint32_t width, uint32_t rows, uint32_t n, int threshold, uint8_t* out) {
    const int lg = sample_factor_lg(n);
    if (!xrgb || !out || !lg || threshold < 0 || threshold > 256 || !width || !rows) return 0;
    const uint32_t b = 8u / n, bc = (width + b - 1) / b, br = (rows + b - 1) / b;
    memset(out, 0, (size_t)bc * br);
    for (uint32_t y = 0; y < rows; y++)
        for (uint32_t x = 0; x < width; x++) {
            const uint32_t* p = xrgb + (size_t)y * width + x;
            uint32_t c = 0, v;
            if (x > 0 && (v = channel_contrast(*p, p[-1])) > c) c = v;
            if (x + 1 < width && (v = channel_contrast(*p, p[1])) > c) c = v;
            if (y > 0 && (v = channel_contrast(*p, *(p - width))) > c) c = v;
            if (y + 1 < rows && (v = channel_contrast(*p, p[width])) > c) c = v;
            if ((int)c >= threshold) out[(size_t)(y / b) * bc + x / b] = 1;
        }
    return 1;
}
