/* ref_tests.h -- the two hit tests of the host definitions (ao_host.c, cast_host.c, layers_host.c): the primary-hit pass's evaluation of its
 * winner (whitted_gbuffer.inc: wt_gb_ref_sphere, wt_gb_ref_plane), the same operations in C, in one place.  Internal, `static inline`: every
 * file that includes it is built with -ffp-contract=off and the functions inherit that per translation unit, so every float32 operation below
 * is rounded once. */
#ifndef REF_TESTS_H
#define REF_TESTS_H
#include <math.h>
#include <stdint.h>
#include <string.h>

static inline float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* s = {centre, +-r * r}: 1 = the ray o + t d meets the sphere at *t > 0 */
static inline int ref_sphere(const float o[3], const float d[3], const float s[4], float* t) {
    const float a = dot3(d, d);
    const float v[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
    const float c = dot3(v, v) - fabsf(s[3]);
    const float b = dot3(v, d);
    const float D = b * b + (-(a * c));
    const float sD = sqrtf(D);
    const float t0 = (-b - sD) / a;
    *t = (t0 < 0) ? (-b + sD) / a : t0;
    return !(D < 0) && !(*t <= 0);
}

/* n = the normal, p0 = a point of the plane: 1 = the ray meets it at *t > 0 */
static inline int ref_plane(const float o[3], const float d[3], const float n[4], const float p0[4], float* t) {
    const float w[3] = {p0[0] - o[0], p0[1] - o[1], p0[2] - o[2]};
    const float num = dot3(w, n);
    const float b = dot3(d, n);
    *t = num / b;
    return !(b == 0) && !(*t <= 0);
}

static inline int sign_bit(float f) { uint32_t u; memcpy(&u, &f, 4); return (int)(u >> 31); }

#endif /* REF_TESTS_H */
