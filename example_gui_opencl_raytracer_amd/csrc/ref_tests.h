/* ref_tests.h -- the reference arithmetic of every pass beside the trace launch, as ONE text: the hit tests, a hit's point and normal, the
 * outgoing ray of a path, a point's distance from a surface, the ambient occlusion basis and resolve, a projected pixel's ray.  Compiled twice from this one text, as
 * primary_cull_host.h is: by the C compiler into the host definitions (cast_host.c, layers_host.c, near_host.c, paths_host.c, ao_host.c, projection_host.c)
 * and by the device compiler into the passes held to them bit for bit (whitted_gbuffer/query/cast/layers/near/paths/ao/projection.inc, in the fast
 * and the strict unit).  Only + - * / sqrt, fabs, copysign and comparisons on float32, each rounded once: no fused operation anywhere
 * (`#pragma clang fp contract(off)` in every function that computes a float; the host C files are built with -ffp-contract=off as well), and
 * both device units are built with correctly rounded divide and square root.  So the per-ray arithmetic of host and device is equal by
 * construction; what the bit-equality tests still hold is everything around it (which primitives are tested, in which order, what is stored).
 * The trace kernels' own arithmetic (whitted_trace.inc: wt_sphere_*, wt_plane, wt_reflect, wt_refract), fused in the fast unit on purpose, is
 * not this text and never calls it.
 * Plain C types only; a vector is a ref_v3 by value. */
#ifndef REF_TESTS_H
#define REF_TESTS_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REF_FN static __host__ __device__ __forceinline__
#else
#define REF_FN static inline
#endif
#ifdef __clang__
#define REF_FP _Pragma("clang fp contract(off)")
#else
#define REF_FP
#endif

#define REF_EPSILON 0.001f         /* primitives.cl:5 */
#define REF_DEFAULT_N 1.0f         /* raytracing.cl:7 */

typedef struct { float x, y, z; } ref_v3;

REF_FN ref_v3 ref_mk(float x, float y, float z) { ref_v3 r; r.x = x; r.y = y; r.z = z; return r; }
REF_FN ref_v3 ref_ld(const float* p) { return ref_mk(p[0], p[1], p[2]); }
REF_FN void ref_st(float* p, ref_v3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
REF_FN int sign_bit(float f) { uint32_t u; memcpy(&u, &f, 4); return (int)(u >> 31); }

REF_FN float ref_dot(ref_v3 a, ref_v3 b) { REF_FP return a.x * b.x + a.y * b.y + a.z * b.z; }
REF_FN ref_v3 ref_add(ref_v3 a, ref_v3 b) { REF_FP return ref_mk(a.x + b.x, a.y + b.y, a.z + b.z); }
REF_FN ref_v3 ref_sub(ref_v3 a, ref_v3 b) { REF_FP return ref_mk(a.x - b.x, a.y - b.y, a.z - b.z); }
REF_FN ref_v3 ref_madd(ref_v3 a, float s, ref_v3 b) { REF_FP return ref_mk(a.x * s + b.x, a.y * s + b.y, a.z * s + b.z); }      /* a s + b */
REF_FN float ref_length(ref_v3 v) { REF_FP return sqrtf(ref_dot(v, v)); }
REF_FN ref_v3 ref_normalize(ref_v3 v) { REF_FP const float len = ref_length(v); return ref_mk(v.x / len, v.y / len, v.z / len); }

/* ---- the sphere {c, w = +-r r} against the ray o + t d, in three pieces: the origin's invariant, the discriminant half, the root half ---- */
/* v = o - c: cc = v.v - r r */
REF_FN float ref_sphere_cc(ref_v3 v, float w) { REF_FP return ref_dot(v, v) - fabsf(w); }
/* a = d.d: b = v.d and D = b b - a cc; 0 = the ray's line misses the sphere (the verdict is then `no hit` whatever the roots are) */
REF_FN int ref_sphere_disc(ref_v3 v, float cc, ref_v3 d, float a, float* b, float* D) {
    REF_FP
    *b = ref_dot(v, d);
    *D = *b * *b + (-(a * cc));
    return !(*D < 0);
}
/* the nearer root, or the farther one where the nearer lies behind the origin */
REF_FN float ref_sphere_root(float b, float D, float a) {
    REF_FP
    const float sD = sqrtf(D);
    const float t0 = (-b - sD) / a;
    return (t0 < 0) ? (-b + sD) / a : t0;
}
/* 1 = the ray meets the sphere at *t > 0: the host definitions' test, and the primary-hit pass's of its winner */
REF_FN int ref_sphere(ref_v3 o, ref_v3 d, ref_v3 c, float w, float* t) {
    float b, D;
    const float a = ref_dot(d, d);
    const ref_v3 v = ref_sub(o, c);
    const int ok = ref_sphere_disc(v, ref_sphere_cc(v, w), d, a, &b, &D);
    *t = ref_sphere_root(b, D, a);
    return ok && !(*t <= 0);
}
/* a hit at t is a candidate of a query whose ray ends at tmax */
REF_FN int ref_candidate(float t, float tmax) { return !(t <= 0) && t <= tmax; }
/* the query form, v, cc and a already taken: 1 = a candidate at *t.  D < 0 leaves before the roots. */
REF_FN int ref_sphere_query(ref_v3 v, float cc, ref_v3 d, float a, float tmax, float* t) {
    float b, D;
    if (!ref_sphere_disc(v, cc, d, a, &b, &D)) return 0;
    *t = ref_sphere_root(b, D, a);
    return ref_candidate(*t, tmax);
}

/* ---- the plane of normal n through p0, in two pieces: the numerator (the origin's invariant) and the rest ---- */
REF_FN float ref_plane_num(ref_v3 o, ref_v3 n, ref_v3 p0) { return ref_dot(ref_sub(p0, o), n); }
REF_FN int ref_plane_rest(float num, ref_v3 n, ref_v3 d, float* t) {
    REF_FP
    const float b = ref_dot(d, n);
    *t = num / b;
    return !(b == 0) && !(*t <= 0);
}
/* 1 = the ray meets the plane at *t > 0 */
REF_FN int ref_plane(ref_v3 o, ref_v3 d, ref_v3 n, ref_v3 p0, float* t) { return ref_plane_rest(ref_plane_num(o, n, p0), n, d, t); }

/* ---- a hit: its point, its normal (g = the plane's normal, never flipped toward the ray, or the sphere's centre), the point shading uses
 *      (primitives.cl:339, 357) ---- */
REF_FN ref_v3 ref_hit_point(ref_v3 o, ref_v3 d, float t) { return ref_madd(d, t, o); }
REF_FN ref_v3 ref_hit_normal(int plane, ref_v3 point, ref_v3 g) { return plane ? g : ref_normalize(ref_sub(point, g)); }
REF_FN ref_v3 ref_hit_offset(ref_v3 point, ref_v3 n) { return ref_madd(n, REF_EPSILON, point); }

/* ---- proximity: how far a point p is from a surface, and the surface's nearest point (the proximity queries: near_host.c, whitted_near.inc) ---- */
/* the sphere or light {c, q = +-r r}, v = p - c: d = |v| - sqrt(|q|), signed, negative inside */
REF_FN float ref_near_sphere(ref_v3 v, float q) { REF_FP return ref_length(v) - sqrtf(fabsf(q)); }
/* the plane of normal n through p0, a two-sided sheet: s = (p - p0).n, d = |s| */
REF_FN float ref_near_plane_s(ref_v3 p, ref_v3 n, ref_v3 p0) { return ref_dot(ref_sub(p, p0), n); }
/* a surface at distance d is a candidate of a probe that reaches `reach` (a NaN on either side is none) */
REF_FN int ref_near_candidate(float d, float reach) { return d <= reach; }
/* the sphere's normal toward p, N = v / |v|, and its nearest point c + N r; at the centre both are the NaNs this computes */
REF_FN void ref_near_sphere_point(ref_v3 p, ref_v3 c, float q, ref_v3* N, ref_v3* point) {
    REF_FP
    *N = ref_normalize(ref_sub(p, c));
    *point = ref_madd(*N, sqrtf(fabsf(q)), c);
}
/* the plane's nearest point p - n s (n taken for unit, as the reference's shading takes it) */
REF_FN ref_v3 ref_near_plane_point(ref_v3 p, ref_v3 n, float s) { REF_FP return ref_mk(p.x - n.x * s, p.y - n.y * s, p.z - n.z * s); }

/* ---- paths: what becomes of a hit (raytracing.cl:139-179 without the weights) ---- */
/* the four words of a 96-byte sphere or plane record that decide where a path goes: byte 64 = offset 32 of its material */
typedef struct { uint32_t transperent, dielectric; float n, reflectivity; } ref_material;

/* primitives.cl:127-130 */
REF_FN ref_v3 ref_reflect(ref_v3 i, ref_v3 n) {
    REF_FP
    const float k = 2 * -ref_dot(n, i);
    return ref_mk(i.x + n.x * k, i.y + n.y * k, i.z + n.z * k);
}
/* primitives.cl:132-144, `i` taken for unit: 0 = total internal reflection (the reference's NaN vector; a NaN x from NaN terms counts as it) */
REF_FN int ref_refract(float n1, float n2, ref_v3 i, ref_v3 nrm, ref_v3* out) {
    REF_FP
    const float n = n1 / n2;
    const float cosI = -ref_dot(nrm, i);
    const float sinT2 = n * n * (1.0f - cosI * cosI);
    if (sinT2 > 1.0f) return 0;
    const float w = n * cosI - sqrtf(1.0f - sinT2);
    *out = ref_mk(i.x * n + nrm.x * w, i.y * n + nrm.y * w, i.z * n + nrm.z * w);
    return !(out->x != out->x);
}
/* a path ends on a surface that neither reflects nor transmits, unless every surface is followed (a light ends it before its words are read) */
REF_FN int ref_path_stops(const ref_material* m, int all_surfaces) {
    return !all_surfaces && m->reflectivity == 0 && !m->dielectric && !m->transperent;
}
/* The ray (*o, *d) that leaves a surface of material m, hit along `dir` with normal nrm; p = ref_hit_offset of the hit; *n1 = the path's
 * refractive index, updated.  The reflected ray from p, or -- `transmit`, through a transparent surface -- the refracted one: from 2 EPSILON
 * behind p when entering, against the negated normal when leaving; on total internal reflection the reflected ray stays and n1 with it. */
REF_FN void ref_bounce(ref_v3 p, ref_v3 nrm, ref_v3 dir, const ref_material* m, int transmit, float* n1, ref_v3* o, ref_v3* d) {
    REF_FP
    *o = p;
    *d = ref_reflect(dir, nrm);
    if (transmit && m->transperent) {
        const float n2 = (*n1 == REF_DEFAULT_N) ? m->n : REF_DEFAULT_N;
        const int entering = *n1 < n2;
        const float e2 = 2 * REF_EPSILON;
        ref_v3 through;
        if (ref_refract(*n1, n2, dir, entering ? nrm : ref_mk(nrm.x * -1.0f, nrm.y * -1.0f, nrm.z * -1.0f), &through)) {
            if (entering) *o = ref_mk(p.x - nrm.x * e2, p.y - nrm.y * e2, p.z - nrm.z * e2);
            *d = through;
            *n1 = n2;
        }
    }
}

/* ---- ambient occlusion: the tangent basis of a normal, a table direction rotated into it, and the integers of the resolve ---- */
REF_FN void ref_ao_basis(ref_v3 n, ref_v3* t, ref_v3* u) {
    REF_FP
    const float sg = copysignf(1.0f, n.z);
    const float a = -1.0f / (sg + n.z);
    const float b = n.x * n.y * a;
    *t = ref_mk(1.0f + sg * n.x * n.x * a, sg * b, -sg * n.x);
    *u = ref_mk(b, sg + n.y * n.y * a, -n.y);
}
REF_FN ref_v3 ref_ao_dir(ref_v3 t, ref_v3 u, ref_v3 n, float lx, float ly, float lz) {
    REF_FP
    return ref_mk(t.x * lx + u.x * ly + n.x * lz, t.y * lx + u.y * ly + n.y * lz, t.z * lx + u.z * ly + n.z * lz);
}
/* S open rays among m pixels of K rays each -> the grey level 0..255 under `strength` (0..256) */
REF_FN uint32_t ref_ao_level(uint32_t S, uint32_t m, uint32_t K, uint32_t strength) {
    const uint32_t v = (255u * S + ((m * K) >> 1)) / (m * K);
    return 255u - (((255u - v) * strength + 128u) >> 8);
}
REF_FN uint32_t ref_ao_grey(uint32_t vs) { return vs * 0x010101u; }
REF_FN uint32_t ref_ao_compose(uint32_t frame, uint32_t vs) {
    uint32_t c = 0u;
    for (int shift = 0; shift < 24; shift += 8) c |= ((((frame >> shift) & 255u) * vs + 127u) / 255u) << shift;
    return c;
}

/* ---- camera models: the image-plane vector of pixel (x, y) (raygen.cl:13-17) -- the pinhole normalises it (ref_normalize), the orthographic
 *      view adds it to the origin; the panorama's vector is ref_madd(column.xyz, row.x, row.yzw), normalised ---- */
REF_FN ref_v3 ref_image_plane(ref_v3 corner, ref_v3 right, ref_v3 up, float w_factor, float h_factor, uint32_t x, uint32_t y) {
    REF_FP
    const float w = (float)x;
    const float h = (float)y;
    return ref_mk(corner.x + right.x * w_factor * w - up.x * h_factor * h, corner.y + right.y * w_factor * w - up.y * h_factor * h,
                  corner.z + right.z * w_factor * w - up.z * h_factor * h);
}

#endif /* REF_TESTS_H */
