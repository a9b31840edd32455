/* bounce_cull_host.h -- the bounce cull table (include/hip_wrap_ext.h: clw_host_bounce_cull): a SECOND byte per 8x8 tile of a tiled launch of
 * the pinhole camera, beside the byte of primary_cull_host.h and one segment further along the path:
 *   bits 0-3 (WT_BC_SHADOW << k): no shadow ray of the tile's FIRST shade can have D >= 0 in wt_shadow_disc for any scene sphere i with
 *                                 i mod 4 = k, whichever light it samples,
 *   bit 4 (WT_BC_REFL_SPHERES):   no ray of the tile's SECOND loop iteration can have D >= 0 in wt_sphere_disc for any scene sphere,
 *   bit 5 (WT_BC_REFL_LIGHTS):    the same for every light sphere,
 * so that wt_trace_cull skips those tests (whitted_trace.inc: wt_shadow_batch; whitted_hit.inc).  A skipped test fails in every lane: the rule
 * only has to be CONSERVATIVE.  wt_bc_tile is THE arithmetic, compiled twice from this text like wt_cull_tile and under the same discipline:
 * double precision, only + - * / sqrt fabs and comparisons, never contracted, a NaN anywhere leaves the bits clear.
 *
 * Precondition (else the byte is 0).  Bit 0 of the primary byte is set: no primary ray of the tile meets a sphere, so each meets a plane or
 * the sky.  With v the UNNORMALISED direction of a pixel (wt_cull_dir; the tile's v fill the parallelogram of its four corner pixels),
 * a_i = (p0_i - o).n_i and b_i(v) = v.n_i, plane i is hit at t_i = a_i / b_i(v) (in units of 1/|v|) when that is positive.  b_i is LINEAR in v,
 * so its sign and its smallest magnitude over the tile are taken at the corners: a plane is "hit by all" when a_i b_i > 0 at the four corners
 * and the centre with |b_i| >= |v| |n_i| / 64 (clear of grazing) and |a_i| clear of its own float32 rounding, "hit by none" when a_i b_i < 0
 * there with the same clearances; any plane that is neither -- two planes meeting inside the tile's view of one of them, a horizon -- leaves
 * the byte 0.  Between two planes hit by all, t_j < t_i  <=>  |a_j| |b_i(v)| - |a_i| |b_j(v)| < 0, again linear in v: the corners decide the
 * interior.  The rule asks -(that) > WT_BC_ORDER Vmax |n_i| |n_j| T at the corners (Vmax the longest corner v, T a bound of both distances
 * plus both |p0 - o|); dividing by |v| <= Vmax and by |b_i(u)| |b_j(u)| <= |n_i| |n_j| for the unit direction u, t_i - t_j >= 1e-3 T for every
 * pixel, against float32 errors of the two quotients below 64 (3e-7 t + 4e-7 |p0 - o|) each.  So ONE plane j is the first hit of every pixel,
 * in the kernel's arithmetic too.  Its normal must be unit: | |n_j|^2 - 1 | <= 2e-6.
 *
 * Footprint.  v -> o + (a_j / b_j(v)) v maps the parallelogram to the plane projectively with a denominator that keeps its sign, so it maps
 * the convex hull of the corners to the convex hull of the four corner hits h_k: every hit of the tile lies in the ball around their mean
 * with R0 = the farthest corner.  The kernel's shading point is ip = (o + t d) + WT_EPSILON n with float32 d (off the pixel's exact direction
 * by < 1e-6 rad: the hit moves by < 1e-6 t / cos), float32 t (num of three roundings on terms of size |p0| + |o|, b of three, a quotient: off
 * by < (3e-7 t + 4e-7 (|p0| + |o|)) / cos) and two fmas (ulps of |ip|): together below slack = WT_BC_POS (tmax + |o| + |p0|) / mincos with
 * mincos >= 1/64 the smallest corner |b_j| / (|v| |n_j|).  So ip lies in B(c_q, R_q), c_q = mean + eps n, R_q = R0 + slack + 2e-6 eps.
 *
 * Bits 0-3.  A shadow ray's line passes through ip and a sample point of a light: within r_l' = r_l (1 + 1e-3) + 1e-6 |c_l - c_q| of the
 * light's centre (its hardware sine and cosine, and the rounding of the sum).  A line through p in B(c_q, R_q) and q in B(c_l, r_l') has its point of parameter
 * s, (1 - s) p + s q, within tube(s) = |1 - s| R_q + |s| r_l' of the axis point c_q + s (c_l - c_q), for EVERY real s: wt_shadow_disc tests
 * the line, behind the surface and beyond the light too.  Sphere (c, r) is clear of all those lines when
 *     g(s) = |c - axis(s)| - tube(s)  >  r (1 + WT_CULL_REL) + WT_CULL_SIN_ABS (|c - c_q| + R_q)        for all s.
 * |c - axis(s)| is convex and the tube is linear on each of s <= 0, 0 <= s <= 1, s >= 1, so g is convex on each: its minimum there is at the
 * stationary point of sqrt(h^2 + x^2) -+ kappa x, x = kappa h / sqrt(1 - kappa^2), clamped into the piece -- three evaluations.  The balls
 * must be apart (R_q + r_l' < |c_l - c_q| / 2: kappa < 1/2) or no bit is set.  The margin is r19's: the line stays r + delta |v| from the
 * centre, sin delta = sin 3e-3, so with sin alpha = r / |v|, sin phi >= sin alpha + sin delta and D / |v|^2 = sin^2 alpha - sin^2 phi
 * <= -sin^2 delta = -8.99997e-6
 * for the exact line; the float32 roundings of wt_shadow_pre / wt_shadow_disc are those listed in primary_cull_host.h (the direction has just
 * been normalised: a = 1 +- 3e-7), below 4e-6.  The position error of ip is inside R_q, not in the margin.  An empty residue class has its
 * bit set; so has every class when there is no light (no shadow ray exists).
 *
 * Bits 4-5.  Plane j's material is not transparent and the launch depth is >= 2: no child is pushed, and every lane alive in the second loop
 * iteration traces d' = d - 2 (d.n) n from ip.  The mirror image of the primary line passes through the VIRTUAL origin o' = o mirrored in
 * the plane and through the hit; the traced line is parallel to it and displaced by |ip - hit| <= eps (1 + 2e-6) + slack =: grow.  So r19's
 * cone argument applies from o' with the cone through the four corner hits and every radius enlarged by grow -- but NOT its margin as it
 * stands.  The kernel evaluates D from v = ip - c, so its roundings scale with |c - ip|^2, not with L_o^2 = |c - o'|^2, and a primitive near
 * o' seen from a far footprint has |c - ip| >> L_o.  So the margin is stated as a distance against Lmax = |c - c_q| + R_q >= |c - ip|: with
 * sin alpha' = (r + grow)(1 + WT_CULL_REL) / L_o and the cone rule phi >= h + alpha' + delta_e, the virtual line stays L_o sin(alpha' +
 * delta_e) = L_o sin alpha' cos delta_e + L_o cos alpha' sin delta_e from c, the traced line grow less; for sin delta_e <= 0.04,
 * cos delta_e (1 + WT_CULL_REL) >= 1, so dist - r >= L_o cos alpha' sin delta_e =: e and -D = dist^2 - r^2 >= e^2 for the exact line.  The
 * rule takes sin delta_e = sin delta' max(1, Lmax / L_o) / cos alpha' (no bit when that passes 0.04), sin delta' = sin 6e-3, which gives
 * e >= Lmax sin delta' and D / |c - ip|^2 <= -sin^2 delta' = -3.59996e-5 whatever the footprint's distance.  Against it stand, all relative
 * to |c - ip|^2: the 4e-6 of roundings of primary_cull_host.h, and 1.2e-5 because n is unit only to 1e-6, which turns d' by up to 4e-6 rad
 * and moves |d'|^2 by up to 8e-6 while the kernel takes a = 1.  (For a plane whose normal is exactly unit only the roundings of wt_reflect
 * remain, below 1e-6 of D / |c - ip|^2: the tests, whose planes are such, hold WT_BC_REFL_HELD; for the shadow lines the float32 direction
 * moves sin^2 phi by < 2e-7: WT_BC_SHADOW_HELD.)
 * Never set: anything when a term is not finite, when the primary byte lacks bit 0, or when a square -- |c - o'|^2, Lmax^2, r^2 -- could
 * overflow float32 (1e37). */
#ifndef BOUNCE_CULL_HOST_H
#define BOUNCE_CULL_HOST_H
#include "primary_cull_host.h"

#define WT_BC_SHADOW 1u                 /* << k, k = sphere index mod 4 */
#define WT_BC_REFL_SPHERES 16u
#define WT_BC_REFL_LIGHTS 32u
#define WT_BC_PART_SHADOW 1u            /* clw_ext_set_bounce_cull: which parts a table carries */
#define WT_BC_PART_REFL 2u
#define WT_BC_EPS 0.001f                /* WT_EPSILON of the trace kernel (whitted_trace.inc holds them equal) */
#define WT_BC_GRAZE 0.015625            /* 1/64 */
#define WT_BC_ORDER 1e-3
#define WT_BC_POS 2e-6
#define WT_BC_SIN_ABS 0.0059999640000648   /* sin(6e-3) */
#define WT_BC_SIN_EFF_MAX 0.04          /* the enlarged margin's sine at most (cos of it times 1 + WT_CULL_REL stays >= 1) */
#define WT_BC_SHADOW_HELD 8.8e-6         /* -D / |c - ip|^2 at least, in float64 on the kernel's float32 ip and direction, under a shadow bit */
#define WT_BC_REFL_HELD 3.5e-5          /* ... under a reflected bit over a plane whose normal is exactly unit */
#define WT_BC_MAX_PLANES 8u             /* more planes than this: no bits (the per-plane terms live in registers on the device) */

/* the scene as the builder reads it: the prepared stream (whitted_params.h) and, for the planes' `transparent` word, the raw 96-byte records */
typedef struct {
    const float* spheres; const float* planes; const float* lights;      /* geom, geom + 4 ns, geom + 4 (ns + 2 np) */
    const uint32_t* planes_raw;                                          /* word 24 i + 16 = plane i's material.transparent */
    uint32_t ns, np, nl, depth;
} wt_bc_scene;

WT_CULL_FN double wt_bc_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* 1 = sphere (c, r2) is clear of every line through B(cq, Rq) and B(cl, rl) (the header's g(s) test) */
WT_CULL_FN int wt_bc_lines_clear(const double c[3], double r2, const double cq[3], double Rq, const double cl[3], double rl) {
    const double e[3] = {cl[0] - cq[0], cl[1] - cq[1], cl[2] - cq[2]}, w[3] = {c[0] - cq[0], c[1] - cq[1], c[2] - cq[2]};
    const double L2 = wt_bc_dot(e, e), W2 = wt_bc_dot(w, w);
    if (!wt_cull_finite(L2) || !wt_cull_finite(W2) || !wt_cull_finite(r2)) return 0;
    if (!(W2 < WT_CULL_F32_MAX) || !(r2 < WT_CULL_F32_MAX) || !(L2 > 0.0)) return 0;
    const double L = sqrt(L2), W = sqrt(W2);
    const double k1 = (Rq + rl) / L, k2 = (rl - Rq) / L;
    if (!(k1 < 0.5)) return 0;                                          /* (|k2| <= k1) */
    const double u0 = wt_bc_dot(w, e) / L;                              /* the centre's foot on the axis, as a length from cq */
    double h2 = W2 - u0 * u0;
    if (!(h2 > 0.0)) h2 = 0.0;
    const double h = sqrt(h2);
    const double need = sqrt(r2) * (1.0 + WT_CULL_REL) + WT_CULL_SIN_ABS * (W + Rq);
    const double x1 = k1 * h / sqrt(1.0 - k1 * k1), x2 = k2 * h / sqrt(1.0 - k2 * k2);
    double u[3] = {u0 - x1, u0 + x2, u0 + x1};                          /* the stationary points of s <= 0, 0 <= s <= 1, s >= 1 */
    if (u[0] > 0.0) u[0] = 0.0;
    if (u[1] < 0.0) u[1] = 0.0;
    if (u[1] > L) u[1] = L;
    if (u[2] < L) u[2] = L;
    for (int p = 0; p < 3; p++) {
        const double x = u[p] - u0;
        const double g = sqrt(h2 + x * x) - (fabs(L - u[p]) * Rq + fabs(u[p]) * rl) / L;
        if (!(g > need)) return 0;
    }
    return 1;
}

/* wt_cull_group_clear with every radius enlarged by `grow` and the margin delta_e, stated against the footprint B(cq, Rq) (the header's bits 4-5) */
WT_CULL_FN int wt_bc_group_clear(const float* geom, uint32_t n, uint32_t stride, const double o[3], const double ax[3], double ch, double sh, double grow,
                                 const double cq[3], double Rq) {
    for (uint32_t i = 0; i < n; i++) {
        const float* s = geom + (size_t)stride * i;
        const double w[3] = {(double)s[0] - o[0], (double)s[1] - o[1], (double)s[2] - o[2]};
        const double q[3] = {(double)s[0] - cq[0], (double)s[1] - cq[1], (double)s[2] - cq[2]};
        const double r2 = fabs((double)s[3]);
        const double L2 = wt_bc_dot(w, w);
        const double Lmax = sqrt(wt_bc_dot(q, q)) + Rq;                   /* >= |c - ip| for every shading point of the tile */
        if (!wt_cull_finite(L2) || !wt_cull_finite(r2) || !wt_cull_finite(Lmax)) return 0;
        if (!(L2 < WT_CULL_F32_MAX) || !(r2 < WT_CULL_F32_MAX) || !(Lmax * Lmax < WT_CULL_F32_MAX)) return 0;
        const double r = sqrt(r2) + grow;
        if (!(L2 > r * r * (1.0 + WT_CULL_REL))) return 0;
        const double L = sqrt(L2);
        const double cphi = fabs(wt_bc_dot(ax, w)) / L;
        const double sa = (r / L) * (1.0 + WT_CULL_REL);
        if (!(sa < 1.0)) return 0;
        const double ca = sqrt(1.0 - sa * sa);
        const double far_ = Lmax > L ? Lmax / L : 1.0;
        const double sd = WT_BC_SIN_ABS * far_ / ca;                      /* sin delta_e */
        if (!(sd <= WT_BC_SIN_EFF_MAX)) return 0;
        const double cd = sqrt(1.0 - sd * sd);
        const double c1 = ch * ca - sh * sa, s1 = sh * ca + ch * sa;
        const double cb = c1 * cd - s1 * sd;
        if (!(c1 > 0.0 && cb > 0.0 && cphi < cb)) return 0;
    }
    return 1;
}

/* The bounce byte of tile (tcol, trow); `prim` = the tile's primary byte (wt_cull_tile); `parts` = WT_BC_PART_* to compute.  The caller has
 * checked wt_cull_view_ok and that the tile has a pixel. */
WT_CULL_FN uint8_t wt_bc_tile(const wt_cull_view* V, uint32_t tcol, uint32_t trow, uint8_t prim, const wt_bc_scene* S, uint32_t parts) {
    if (!(prim & WT_CULL_SPHERES) || S->np == 0u || S->np > WT_BC_MAX_PLANES || (parts & 3u) == 0u) return 0;
    const uint32_t x0 = tcol * 8u, y0l = trow * 8u;
    const uint32_t x1 = x0 + 7u < V->width ? x0 + 7u : V->width - 1u;
    const uint32_t y1l = y0l + 7u < V->rows ? y0l + 7u : V->rows - 1u;
    const double gy0 = V->band_stride > 1u ? (double)(((uint64_t)trow * V->band_stride + V->band_phase) * 8u) : (double)V->row_offset + (double)y0l;
    const double gy1 = gy0 + (double)(y1l - y0l);
    const double fx0 = (double)x0, fx1 = (double)x1;
    const double o[3] = {(double)V->origin[0], (double)V->origin[1], (double)V->origin[2]};
    /* the four corners and the centre: unnormalised directions and their lengths */
    double v[5][3], vl[5], vmax = 0.0;
    for (int k = 0; k < 5; k++) {
        if (k < 4) wt_cull_dir(V, (k & 1) ? fx1 : fx0, (k & 2) ? gy1 : gy0, v[k]);
        else wt_cull_dir(V, 0.5 * (fx0 + fx1), 0.5 * (gy0 + gy1), v[k]);
        vl[k] = sqrt(wt_bc_dot(v[k], v[k]));
        if (!(vl[k] > 0.0) || !wt_cull_finite(vl[k])) return 0;
        if (vl[k] > vmax) vmax = vl[k];
    }
    /* every plane: hit by all (its distance bound T_i) or by none, else no bits */
    double a[WT_BC_MAX_PLANES], nlen[WT_BC_MAX_PLANES], T[WT_BC_MAX_PLANES], po[WT_BC_MAX_PLANES], tc[WT_BC_MAX_PLANES];
    int hit[WT_BC_MAX_PLANES], j = -1;
    for (uint32_t i = 0; i < S->np; i++) {
        const float* g = S->planes + 8u * (size_t)i;
        const double n[3] = {(double)g[0], (double)g[1], (double)g[2]};
        const double d[3] = {(double)g[4] - o[0], (double)g[5] - o[1], (double)g[6] - o[2]};
        nlen[i] = sqrt(wt_bc_dot(n, n)); po[i] = sqrt(wt_bc_dot(d, d)); a[i] = wt_bc_dot(d, n);
        if (!(nlen[i] > 0.0) || !wt_cull_finite(nlen[i]) || !wt_cull_finite(po[i]) || !(po[i] < 1e18)) return 0;
        if (!(fabs(a[i]) > 1e-4 * po[i] * nlen[i])) return 0;            /* the origin on the plane, to float32 */
        int pos = 0, neg = 0;
        double bmin = 0.0;
        for (int k = 0; k < 5; k++) {
            const double b = wt_bc_dot(v[k], n);
            if (!(fabs(b) >= WT_BC_GRAZE * vl[k] * nlen[i])) return 0;   /* grazing, or NaN */
            if (a[i] * b > 0.0) pos++; else neg++;
            if (k == 0 || fabs(b) < bmin) bmin = fabs(b);
            if (k == 4) tc[i] = fabs(a[i]) * vl[4] / fabs(b);
        }
        if (pos != 5 && neg != 5) return 0;
        hit[i] = pos == 5;
        T[i] = fabs(a[i]) * vmax / bmin;
        if (hit[i] && (j < 0 || tc[i] < tc[j])) j = (int)i;
    }
    if (j < 0) return 0;                                                 /* the sky */
    const float* gj = S->planes + 8u * (size_t)j;
    const double nj[3] = {(double)gj[0], (double)gj[1], (double)gj[2]};
    for (uint32_t i = 0; i < S->np; i++) {
        if ((int)i == j || !hit[i]) continue;
        const float* g = S->planes + 8u * (size_t)i;
        const double n[3] = {(double)g[0], (double)g[1], (double)g[2]};
        const double bound = WT_BC_ORDER * vmax * nlen[i] * nlen[j] * (T[i] + T[j] + po[i] + po[j]);
        for (int k = 0; k < 5; k++)
            if (!(fabs(a[i]) * fabs(wt_bc_dot(v[k], nj)) - fabs(a[j]) * fabs(wt_bc_dot(v[k], n)) > bound)) return 0;
    }
    if (!(fabs(nlen[j] * nlen[j] - 1.0) <= 2e-6)) return 0;
    /* the footprint */
    double h[4][3], m[3] = {0.0, 0.0, 0.0}, tmax = 0.0, mincos = 1.0;
    for (int k = 0; k < 4; k++) {
        const double b = wt_bc_dot(v[k], nj), t = a[j] / b;
        for (int c = 0; c < 3; c++) { h[k][c] = o[c] + t * v[k][c]; m[c] += 0.25 * h[k][c]; }
        if (t * vl[k] > tmax) tmax = t * vl[k];
        const double cs = fabs(b) / (vl[k] * nlen[j]);
        if (cs < mincos) mincos = cs;
    }
    double R0 = 0.0;
    for (int k = 0; k < 4; k++) {
        const double d[3] = {h[k][0] - m[0], h[k][1] - m[1], h[k][2] - m[2]};
        const double r = sqrt(wt_bc_dot(d, d));
        if (!wt_cull_finite(r)) return 0;
        if (r > R0) R0 = r;
    }
    const double p0l = sqrt((double)gj[4] * (double)gj[4] + (double)gj[5] * (double)gj[5] + (double)gj[6] * (double)gj[6]);
    const double slack = WT_BC_POS * (tmax + sqrt(wt_bc_dot(o, o)) + p0l) / mincos;
    const double eps = (double)WT_BC_EPS;
    const double cq[3] = {m[0] + eps * nj[0], m[1] + eps * nj[1], m[2] + eps * nj[2]};
    const double Rq = R0 + slack + 2e-6 * eps;
    if (!wt_cull_finite(Rq) || !wt_cull_finite(cq[0] + cq[1] + cq[2])) return 0;
    uint8_t bits = 0;
    if (parts & WT_BC_PART_SHADOW) {
        unsigned clear = 15u;
        for (uint32_t i = 0; i < S->ns && clear; i++) {
            if (!((clear >> (i & 3u)) & 1u)) continue;
            const float* s = S->spheres + 4u * (size_t)i;
            const double c[3] = {(double)s[0], (double)s[1], (double)s[2]};
            for (uint32_t l = 0; l < S->nl; l++) {
                const float* lg = S->lights + 8u * (size_t)l;
                const double cl[3] = {(double)lg[0], (double)lg[1], (double)lg[2]};
                const double e[3] = {cl[0] - cq[0], cl[1] - cq[1], cl[2] - cq[2]};
                const double rl = fabs((double)lg[7]) * (1.0 + WT_CULL_REL) + 1e-6 * sqrt(wt_bc_dot(e, e));
                if (!wt_bc_lines_clear(c, fabs((double)s[3]), cq, Rq, cl, rl)) { clear &= ~(1u << (i & 3u)); break; }
            }
        }
        bits |= (uint8_t)clear;
    }
    if ((parts & WT_BC_PART_REFL) && S->depth >= 2u && S->planes_raw[24u * (size_t)j + 16u] == 0u) {
        const double f = 2.0 * a[j] / (nlen[j] * nlen[j]);               /* o' = o + 2 ((p0 - o).n / n.n) n */
        const double ov[3] = {o[0] + f * nj[0], o[1] + f * nj[1], o[2] + f * nj[2]};
        double ax[3] = {m[0] - ov[0], m[1] - ov[1], m[2] - ov[2]};
        const double al = sqrt(wt_bc_dot(ax, ax));
        int ok = al > 0.0 && wt_cull_finite(al);
        double ch = 1.0;
        for (int k = 0; k < 4 && ok; k++) {
            const double u[3] = {h[k][0] - ov[0], h[k][1] - ov[1], h[k][2] - ov[2]};
            const double ul = sqrt(wt_bc_dot(u, u));
            const double c = wt_bc_dot(ax, u) / (al * ul);
            if (!(c >= 0.5)) ok = 0;
            else if (c < ch) ch = c;
        }
        if (ok) {
            for (int c = 0; c < 3; c++) ax[c] = ax[c] / al;
            double sh = sqrt(1.0 - ch * ch) * (1.0 + WT_CULL_REL);
            if (sh < 1.0) {
                ch = sqrt(1.0 - sh * sh);
                const double grow = eps * (1.0 + 2e-6) + slack;
                if (wt_bc_group_clear(S->spheres, S->ns, 4u, ov, ax, ch, sh, grow, cq, Rq)) bits |= WT_BC_REFL_SPHERES;
                if (wt_bc_group_clear(S->lights, S->nl, 8u, ov, ax, ch, sh, grow, cq, Rq)) bits |= WT_BC_REFL_LIGHTS;
            }
        }
    }
    return bits;
}

#ifdef __cplusplus
extern "C" {
#endif
/* both tables of a launch from PREPARED geometry: `prim` (may be NULL) receives the primary bytes, `out` the bounce bytes -> tiles written, 0 =
 * refused.  A view with a term that is not finite writes zeros. */
uint32_t wt_bc_table(const wt_cull_view* V, const wt_bc_scene* S, uint32_t parts, uint8_t* prim, uint8_t* out);
#ifdef __cplusplus
}
#endif
#endif /* BOUNCE_CULL_HOST_H */
