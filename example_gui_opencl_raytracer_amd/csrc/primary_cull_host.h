/* primary_cull_host.h -- the primary-ray cull table (include/hip_wrap_ext.h: clw_host_primary_cull): one byte per 8x8 tile of a tiled launch
 * of the pinhole camera,
 *   bit 0 (WT_CULL_SPHERES): no primary ray of the tile can have D >= 0 in the discriminant half of the sphere test (wt_sphere_disc) for ANY
 *                            scene sphere,
 *   bit 1 (WT_CULL_LIGHTS):  the same for every light sphere,
 * so that the trace kernel's first loop iteration skips the whole group (whitted_hit.inc).  Skipping a test that fails in every lane changes
 * no bit of the image; the rule only has to be CONSERVATIVE.
 *
 * wt_cull_tile below is THE arithmetic, compiled twice from this one text: by the C compiler into primary_cull_host.c (the host definition) and
 * by the device compiler into wt_primary_cull_build (whitted_cull.inc).  It is double precision and uses only + - * / sqrt and comparisons, each
 * correctly rounded on both sides and never contracted (-ffp-contract=off in both units), so the two tables agree bit for bit.
 *
 * The rule.  A tile's pixels are columns [x0, x1] and global rows [y0, y1] (clipped to the frame).  Their unnormalised directions
 * v(px, py) = corner + right (w_factor px) - up (h_factor py) fill a planar parallelogram; a cone of half-angle below 90 degrees cuts a plane in
 * a convex region, so the cone around the axis a = v(centre) through the four corner pixels' directions holds all of them: half-angle h, cos h
 * = the smallest a.u_k.  wt_sphere_disc tests the LINE of a ray, not the half-line: a sphere behind the camera has D >= 0 as well.  So with w =
 * centre - origin, L = |w|, the angle phi in [0, 90] between the axis and the line of w (cos phi = |a.w| / L) and the sphere's angular radius
 * alpha (sin alpha = r / L), the sphere is clear of the tile when
 *     phi > h + alpha + delta        <=>   cos phi < cos(h + alpha + delta)  and  cos(h + alpha + delta) > 0,
 * evaluated with the angle-sum formulas on sines and cosines (no inverse function needed), the two sines first enlarged by WT_CULL_REL.
 *
 * The margin delta = WT_CULL_ABS = 3e-3 rad.  For a unit direction d at angle phi_d to the line, D / L^2 = sin^2 alpha - sin^2 phi_d
 * = -sin(phi_d - alpha) sin(phi_d + alpha) <= -sin^2 delta = -9e-6 under the rule (phi_d >= alpha + delta, and phi_d + alpha <= 180 - delta).
 * Against it stand the fp32 roundings of the kernel: wt_primary_dir_xy (seven roundings per component, a sqrt and a divide: the direction
 * turns by < 1e-6 rad, sin^2 moves by < 2e-6), v = o - c (relative 6e-8 per component), c = v.v - r^2 (< 2.4e-7 L^2), b = v.d (< 2e-7 L, so
 * b^2 moves by < 4e-7 L^2), a = d.d = 1 +- 3e-7 taken as 1 by the fast build, the final fma (6e-8): together below 4e-6 L^2, less than half
 * of 9e-6.  (A purely relative margin would not do: around a small distant light h + alpha is a few 1e-3 rad, 1e-3 of it a few 1e-6 rad, and
 * sin delta sin(2 alpha + delta) falls far below the rounding.)  3e-3 rad is two thirds of a tile at 1920 columns and 60 degrees: a ring of
 * one tile around each silhouette stays untested-for, which costs nothing measurable.
 * Never set: a bit whose group holds a sphere with the origin inside or on it (L^2 <= r^2 (1 + WT_CULL_REL)), any bit when a camera term is not
 * finite, a tile whose cone is wider than 60 degrees (cos h < 1/2: no real view), a group with a term that is not finite or with a sphere so
 * far or so large that |c - o|^2 or r^2 reaches 1e37 (in the kernel's float32 v.v would overflow and D be NaN, which HITS).  An EMPTY group has
 * its bit set (nothing to test).  Comparisons are written so that a NaN anywhere leaves the bit clear. */
#ifndef PRIMARY_CULL_HOST_H
#define PRIMARY_CULL_HOST_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define WT_CULL_SPHERES 1u
#define WT_CULL_LIGHTS 2u
#define WT_CULL_REL 1e-3
#define WT_CULL_F32_MAX 1e37                 /* squares beyond this may overflow the kernel's float32 */
#define WT_CULL_COS_ABS 0.9999955000033750   /* cos(3e-3) */
#define WT_CULL_SIN_ABS 0.0029999955000020   /* sin(3e-3) */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WT_CULL_FN static __host__ __device__ __forceinline__
#else
#define WT_CULL_FN static inline
#endif

/* the camera terms of a launch as the kernel reads them (whitted_params.h), the frame's width, and the launch's rows: local row y of the range is
 * global row row_offset + y, or -- band_stride > 1, interleaved 8-row bands -- ((y / 8) band_stride + band_phase) 8 + y % 8 */
typedef struct {
    float corner[3], origin[3], up[3], right[3];
    float w_factor, h_factor;
    uint32_t width, rows, row_offset, band_stride, band_phase;
} wt_cull_view;

WT_CULL_FN int wt_cull_finite(double x) { return x - x == 0.0; }

/* every camera term finite */
WT_CULL_FN int wt_cull_view_ok(const wt_cull_view* V) {
    double s = (double)V->w_factor - (double)V->w_factor + ((double)V->h_factor - (double)V->h_factor);
    for (int a = 0; a < 3; a++)
        s += ((double)V->corner[a] - (double)V->corner[a]) + ((double)V->origin[a] - (double)V->origin[a]) + ((double)V->up[a] - (double)V->up[a]) +
             ((double)V->right[a] - (double)V->right[a]);
    return s == 0.0;
}

/* unnormalised direction of pixel (px, py), px and py possibly half-integers (the tile centre) */
WT_CULL_FN void wt_cull_dir(const wt_cull_view* V, double px, double py, double v[3]) {
    for (int a = 0; a < 3; a++)
        v[a] = ((double)V->corner[a] + (double)V->right[a] * (double)V->w_factor * px) - (double)V->up[a] * (double)V->h_factor * py;
}

/* 1 = every sphere of geom[stride * i + 0..3] = { cx, cy, cz, +-r^2 }, i < n, is clear of the cone (unit axis `ax`, cos h, sin h) */
WT_CULL_FN int wt_cull_group_clear(const float* geom, uint32_t n, uint32_t stride, const double o[3], const double ax[3], double ch, double sh) {
    for (uint32_t i = 0; i < n; i++) {
        const float* s = geom + (size_t)stride * i;
        const double w[3] = {(double)s[0] - o[0], (double)s[1] - o[1], (double)s[2] - o[2]};
        const double r2 = fabs((double)s[3]);
        const double L2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        if (!wt_cull_finite(L2) || !wt_cull_finite(r2)) return 0;
        /* the kernel works in float32 and its rejecting test is `D < 0`: where v.v or r^2 could overflow there, D is inf - inf = NaN and the ray
         * "hits" -- no bit for such a sphere (1e37: a factor 34 below FLT_MAX, above any rounding of the partial sums) */
        if (!(L2 < WT_CULL_F32_MAX) || !(r2 < WT_CULL_F32_MAX)) return 0;
        if (!(L2 > r2 * (1.0 + WT_CULL_REL))) return 0;            /* the origin inside or on the sphere (or L2 = 0) */
        const double L = sqrt(L2);
        const double cphi = fabs(ax[0] * w[0] + ax[1] * w[1] + ax[2] * w[2]) / L;
        double sa = sqrt(r2 / L2) * (1.0 + WT_CULL_REL);
        if (!(sa < 1.0)) return 0;
        const double ca = sqrt(1.0 - sa * sa);
        const double c1 = ch * ca - sh * sa, s1 = sh * ca + ch * sa;                      /* cos, sin of h + alpha */
        const double cb = c1 * WT_CULL_COS_ABS - s1 * WT_CULL_SIN_ABS;                  /* cos of h + alpha + delta */
        if (!(c1 > 0.0 && cb > 0.0 && cphi < cb)) return 0;
    }
    return 1;
}

/* The byte of tile (tcol, trow) of the launch's tile grid; `spheres` = ns float4 { c, +-r^2 }, `lights` = nl PAIRS of float4 whose first is
 * { c, r^2 } (the prepared stream of whitted_params.h).  The caller has checked wt_cull_view_ok and that the tile has a pixel. */
WT_CULL_FN uint8_t wt_cull_tile(const wt_cull_view* V, uint32_t tcol, uint32_t trow, const float* spheres, uint32_t ns, const float* lights, uint32_t nl) {
    const uint32_t x0 = tcol * 8u, y0l = trow * 8u;
    const uint32_t x1 = x0 + 7u < V->width ? x0 + 7u : V->width - 1u;
    const uint32_t y1l = y0l + 7u < V->rows ? y0l + 7u : V->rows - 1u;
    /* (a tile's local rows share their band: 8-row bands start on tile rows) */
    const double gy0 = V->band_stride > 1u ? (double)(((uint64_t)trow * V->band_stride + V->band_phase) * 8u) : (double)V->row_offset + (double)y0l;
    const double gy1 = gy0 + (double)(y1l - y0l);
    const double fx0 = (double)x0, fx1 = (double)x1;
    double ax[3], u[3];
    wt_cull_dir(V, 0.5 * (fx0 + fx1), 0.5 * (gy0 + gy1), ax);
    const double al = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (!(al > 0.0) || !wt_cull_finite(al)) return 0;
    for (int a = 0; a < 3; a++) ax[a] = ax[a] / al;
    double ch = 1.0;
    for (int k = 0; k < 4; k++) {
        wt_cull_dir(V, (k & 1) ? fx1 : fx0, (k & 2) ? gy1 : gy0, u);
        const double ul = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (!(ul > 0.0) || !wt_cull_finite(ul)) return 0;
        const double c = (ax[0] * u[0] + ax[1] * u[1] + ax[2] * u[2]) / ul;
        if (!(c >= 0.5)) return 0;                                  /* wider than 60 degrees, or NaN */
        if (c < ch) ch = c;
    }
    double sh = sqrt(1.0 - ch * ch) * (1.0 + WT_CULL_REL);
    if (!(sh < 1.0)) return 0;
    ch = sqrt(1.0 - sh * sh);
    const double o[3] = {(double)V->origin[0], (double)V->origin[1], (double)V->origin[2]};
    uint8_t bits = 0;
    if (wt_cull_group_clear(spheres, ns, 4u, o, ax, ch, sh)) bits |= WT_CULL_SPHERES;
    if (wt_cull_group_clear(lights, nl, 8u, o, ax, ch, sh)) bits |= WT_CULL_LIGHTS;
    return bits;
}

#ifdef __cplusplus
extern "C" {
#endif
/* tiles of a launch of `width` columns and `rows` rows: ceil(rows / 8) * ceil(width / 8), 0 when either is 0 or the count passes 2^31 */
uint32_t wt_cull_tiles(uint32_t width, uint32_t rows);
/* the table of a launch from PREPARED geometry (the float4 stream of whitted_params.h: `spheres` = geom, `lights` = geom + 4 (ns + 2 np)) ->
 * tiles written, 0 = refused (no tiles, a NULL pointer with a count > 0).  A view with a term that is not finite writes zeros. */
uint32_t wt_cull_table(const wt_cull_view* V, const float* spheres, uint32_t ns, const float* lights, uint32_t nl, uint8_t* out);
#ifdef __cplusplus
}
#endif
#endif /* PRIMARY_CULL_HOST_H */
